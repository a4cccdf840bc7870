// kp1_row_reread_body.inc -- a lane that does not step an env fills its `o` from an observation row that is already in memory, so that the
// whole-tile store that follows has the same surroundings as in the step form (ES_EPISODE_REREADS of kp1_eval_step.inc has the reason: the
// env step's fp32 sums are not contraction-pinned, and the code around the inlined step decides how the compiler fuses them).
// Included as text by eval_step_kernel's episode form and by rollout_run_kernel, each after its own prologue, which declares
//   src (const f32x4*: the row, KP1_OBS_DIM floats, 16-byte aligned) next to the lane's o (float[KP1_OBS_DIM]).
// One text, so the copies cannot drift; text and not a call, see DESIGN section 28.
#pragma unroll
  for (int k = 0; k < KP1_OBS_DIM / 4; ++k) {
    const f32x4 v = src[k];
    o[4 * k] = v.x; o[4 * k + 1] = v.y; o[4 * k + 2] = v.z; o[4 * k + 3] = v.w;
  }
