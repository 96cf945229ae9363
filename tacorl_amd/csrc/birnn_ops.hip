// Layout kernel of the bidirectional ReLU-RNN plan recognition (reference
// networks/plan_encoders/plan_recognition_tanh_net.py: torch nn.RNN(num_layers=2, bidirectional=True, batch_first=True)).
//
// The recurrence runs time-major: one launch per time step covers both directions (two problems of the batched
// GEMMs, time indices s and T-1-s) and reads / writes one [B][2H] slab of the interleaved [T][B][2H] output.  The
// module's input embeddings arrive batch-major ([B*T] rows b*T+t) and its input gradient leaves batch-major; this
// kernel moves rows between the two orders: dst[(i*n_outer + o)][c] = src[(o*n_inner + i)][c].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tacorl_hip.h"
#include "common.h"

__global__ __launch_bounds__(256) void birnn_swap_rows_kernel(const float* __restrict__ src, int ld_src, float* __restrict__ dst,
                                                              int ld_dst, int n_outer, int n_inner, int cols) {
  const long total = (long)n_outer * n_inner * cols;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long)gridDim.x * 256) {
    const int c = (int)(q % cols);
    const long r = q / cols;            // source row o * n_inner + i
    const int i = (int)(r % n_inner), o = (int)(r / n_inner);
    dst[((long)i * n_outer + o) * ld_dst + c] = src[r * ld_src + c];
  }
}

extern "C" int tacorl_birnn_swap_rows(const float* src, int ld_src, float* dst, int ld_dst, int n_outer, int n_inner, int cols,
                                      tacorl_stream_t stream) {
  if (n_outer < 1 || n_inner < 1 || cols < 1 || ld_src < cols || ld_dst < cols || !src || !dst) return TACORL_EINVAL;
  const long total = (long)n_outer * n_inner * cols;
  const int blocks = (int)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256);
  hipLaunchKernelGGL(birnn_swap_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, ld_src, dst, ld_dst, n_outer,
                     n_inner, cols);
  return hipGetLastError() == hipSuccess ? TACORL_OK : TACORL_ELAUNCH;
}
