// kp1_tracker_scratch.inc -- the LDS of a point-curriculum tracker kernel (kp1_ppo.hip), included as text at the top of each of the three:
// the success ring, and the whole-wave path's success bits in episode order with their prefix counts (tracker_block_parallel).
__shared__ int ring[KP1_CURRICULUM_MAX_WINDOW];
__shared__ uint8_t sbit[TRK_BLOCK];
__shared__ uint16_t pfx[TRK_BLOCK + KP1_CURRICULUM_MAX_WINDOW + 1];
const TrackerScratch ws = {sbit, pfx};
