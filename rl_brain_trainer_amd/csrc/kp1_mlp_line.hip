// kp1_mlp_line.hip -- the kernels only a handle with a hyper-parameter line launches (kp1_mlp_hparams_store):
// hparams_store_kernel, mlp_tile_line_kernel<2 / 4> and head_train_kernel<256, true>.
//
// A translation unit is a code object.  Instantiated in kp1_mlp.hip these four kernels grew the sections in front of its .text and moved
// every kernel of that file, and the benchmark, which launches none of the four, read 0.2 - 0.5 % lower.  Here they cannot: kp1_mlp.hip's
// code object is what it was without them (tools/check_device_code.py --digest: disassembly and notes).  The kernels' text is kp1_mlp.hip's own (its device part up to the tile kernels,
// included below; nothing else of it is instantiated, so nothing else of it is emitted here).
#define KP1_MLP_LINE_TU
#include "kp1_mlp.hip"

namespace {
#include "kp1_hparam_line.inc"
}  // namespace

namespace kp1 {
int mlp_line_launch_tile(const void* fused_args, size_t bytes, const float* line, dim3 grid, hipEvent_t start, hipEvent_t stop, hipStream_t stream) {
  if (!fused_args || !line || bytes != sizeof(FusedArgs)) return fail(KP1_ERR_INVALID, "mlp_line_launch_tile: not a FusedArgs block");
  FusedArgs fa;
  std::memcpy(&fa, fused_args, sizeof(fa));
  const size_t lds = sizeof(float) * FU_LDS_FLOATS;
  auto* kernel = fa.inp == 64 ? mlp_tile_line_kernel<2> : mlp_tile_line_kernel<4>;
  HIP_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (start != nullptr) hipExtLaunchKernelGGL(kernel, grid, dim3(FU_NTH), lds, stream, start, stop, 0, fa, line);
  else hipLaunchKernelGGL(kernel, grid, dim3(FU_NTH), lds, stream, fa, line);
  return KP1_OK;
}

int mlp_line_launch_head_train256(const void* head_args, size_t bytes, dim3 grid, size_t lds_bytes, hipStream_t stream) {
  if (!head_args || bytes != sizeof(HeadArgs)) return fail(KP1_ERR_INVALID, "mlp_line_launch_head_train256: not a HeadArgs block");
  HeadArgs a;
  std::memcpy(&a, head_args, sizeof(a));
  auto* kernel = head_train_kernel<256, true>;
  HIP_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  hipLaunchKernelGGL(kernel, grid, dim3(256), lds_bytes, stream, a);
  return KP1_OK;
}

int mlp_line_store(float* table, const float* v, int n_floats, hipStream_t stream) {
  if (!table || !v || n_floats < 1 || n_floats > HPARAM_TABLE_FLOATS) return fail(KP1_ERR_INVALID, "mlp_line_store: 1 .. KP1_MLP_MAX_REPLICAS entries");
  HparamTable t{};
  std::memcpy(t.v, v, sizeof(float) * (size_t)n_floats);
  hipLaunchKernelGGL(hparams_store_kernel, dim3(1), dim3(HPARAM_TABLE_FLOATS), 0, stream, table, t, n_floats);
  HIP_TRY(kp1::launch_status());
  return KP1_OK;
}
}  // namespace kp1
