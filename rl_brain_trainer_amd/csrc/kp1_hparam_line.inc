// kp1_hparam_line.inc -- kp1_mlp_hparams_store's launch (DESIGN.md section 37).  Included by kp1_mlp_line.hip inside its anonymous namespace.
//
// The K entries of a handle's hyper-parameter table (at most KP1_MLP_MAX_REPLICAS x HP_FIELDS floats, 384 bytes) arrive as kernel arguments
// and one thread per float writes them with a plain vector store: stream ordered like any launch, capturable, no copy engine, no caller
// memory read after the call returns.  The kernels that read the table load it at their entry, so a launch queued behind this one sees
// the new values and a launch in front of it the old ones.
constexpr int HPARAM_TABLE_FLOATS = KP1_MLP_MAX_REPLICAS * HP_FIELDS;
struct HparamTable { float v[HPARAM_TABLE_FLOATS]; };

__global__ void __launch_bounds__(HPARAM_TABLE_FLOATS) hparams_store_kernel(float* __restrict__ table, const HparamTable t, int n_floats) {
  const int i = (int)threadIdx.x;
  if (i < n_floats) table[i] = t.v[i];   // i < n_floats <= HPARAM_TABLE_FLOATS: inside both the argument block and the K-entry allocation
}
