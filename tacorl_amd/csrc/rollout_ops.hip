// Rollout-time linear layers for a handful of rows (1 <= R <= 64): y = act(b1 + b2 + x1 W1^T + x2 W2^T) read straight from
// torch's row-major fp32 masters.  One call is a whole ReLU-RNN cell of the action decoder's one-step rollout
// (x1 = the layer's input, x2 = h_{t-1}), or - without x2 - a head projection.
//
// At these row counts the cell is pure weight streaming (R/2 FLOP per byte), so the kernel is a batched GEMV, not a GEMM:
//   - one wave per output neuron (RL_NPW neurons per wave, one after the other); the lanes stride the neuron's weight row
//     with 16-byte loads straight into registers - a scalar head up to the row's first 16-byte boundary, a scalar tail;
//   - a group of RL_G rows of [x1 | x2] is staged in LDS in chunks of RL_KC columns (64 KiB: two workgroups per CU), read
//     back as ds_read_b128 where the weight row's head is empty;
//   - one fp32 FMA accumulator per (neuron, row) and lane, summed over the wave by a fixed xor butterfly.
// Row determinism: the order in which row r's products are added depends on (n, K1, K2, the weight row's alignment) only -
// never on R, on the row's place in its group or on the other rows; there are no atomics and no split of the reduction
// across workgroups.  A row flagged in x2_row_is_zero is staged as zeros and never read from memory (h_0 = 0 of a plan
// that starts at this step, whatever the buffer holds).
#include "../../include/tacorl_hip.h"
#include "common.h"

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? TACORL_OK : TACORL_ELAUNCH)

namespace {

constexpr int RL_G = 8;        // rows per group (tacorl_rows_linear2_group)
constexpr int RL_KC = 2048;    // columns of [x1 | x2] staged at a time
constexpr int RL_WAVES = 4;    // waves per workgroup
constexpr int RL_NPW = 2;      // neurons per wave
constexpr int RL_NPB = RL_WAVES * RL_NPW;
constexpr int RL_MAX_DIM = 1 << 24;

// rows [r0, r0 + RL_G) x columns [c0, c0 + len) of x into xs[g][0 .. len); rows past R and flagged rows become zeros
__device__ __forceinline__ void rl_stage(float* xs, const float* x, int ldx, int c0, int len, int r0, int R,
                                         const unsigned char* zero_flags, int nr) {
  const int tid = threadIdx.x, nt = RL_WAVES * 64;
  for (int g = 0; g < nr; ++g) {
    const int r = r0 + g;
    float* dst = xs + g * RL_KC;
    if (r >= R || (zero_flags != nullptr && zero_flags[r] != 0)) {
      for (int i = tid; i < len; i += nt) dst[i] = 0.f;
      continue;
    }
    const float* src = x + (long)r * ldx + c0;
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
      const int n4 = len >> 2;
      for (int i = tid; i < n4; i += nt) reinterpret_cast<f32x4*>(dst)[i] = reinterpret_cast<const f32x4*>(src)[i];
      for (int i = 4 * n4 + tid; i < len; i += nt) dst[i] = src[i];
    } else {
      for (int i = tid; i < len; i += nt) dst[i] = src[i];
    }
  }
}

// acc[g] += sum_k wrow[k] * xs[g][k] over k in [0, len), this lane's share
template <int NR>
__device__ __forceinline__ void rl_dot(const float* wrow, const float* xs, int len, int lane, float (&acc)[RL_G]) {
  int head = (int)((0 - (reinterpret_cast<uintptr_t>(wrow) >> 2)) & 3);  // floats up to the row's first 16-byte boundary
  head = head < len ? head : len;
  if (lane < head) {
    const float wv = wrow[lane];
#pragma unroll
    for (int g = 0; g < NR; ++g) acc[g] = fmaf(wv, xs[g * RL_KC + lane], acc[g]);
  }
  const int nb = (len - head) >> 2;
  const f32x4* wb = reinterpret_cast<const f32x4*>(wrow + head);
  if (head == 0) {
#pragma unroll 2
    for (int i = lane; i < nb; i += 64) {
      const f32x4 wv = wb[i];
#pragma unroll
      for (int g = 0; g < NR; ++g) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + g * RL_KC + 4 * i);
        acc[g] = fmaf(wv[0], xv[0], acc[g]);
        acc[g] = fmaf(wv[1], xv[1], acc[g]);
        acc[g] = fmaf(wv[2], xv[2], acc[g]);
        acc[g] = fmaf(wv[3], xv[3], acc[g]);
      }
    }
  } else {
#pragma unroll 2
    for (int i = lane; i < nb; i += 64) {
      const f32x4 wv = wb[i];
      const float* xp = xs + head + 4 * i;
#pragma unroll
      for (int g = 0; g < NR; ++g) {
        acc[g] = fmaf(wv[0], xp[g * RL_KC + 0], acc[g]);
        acc[g] = fmaf(wv[1], xp[g * RL_KC + 1], acc[g]);
        acc[g] = fmaf(wv[2], xp[g * RL_KC + 2], acc[g]);
        acc[g] = fmaf(wv[3], xp[g * RL_KC + 3], acc[g]);
      }
    }
  }
  const int t = head + 4 * nb + lane;
  if (t < len) {
    const float wv = wrow[t];
#pragma unroll
    for (int g = 0; g < NR; ++g) acc[g] = fmaf(wv, xs[g * RL_KC + t], acc[g]);
  }
}

struct RowsLinearArgs {
  const float *x1, *w1, *b1, *x2, *w2, *b2;
  const unsigned char* x2_zero;
  float* y;
  int ldx1, K1, ldx2, K2, ldy, R, N, act;
};

template <int NR>
__device__ __forceinline__ void rows_linear2_body(const RowsLinearArgs& a, float* xs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.y * RL_G;
  const int n0 = blockIdx.x * RL_NPB + wave * RL_NPW;
  float acc[RL_NPW][RL_G];
#pragma unroll
  for (int j = 0; j < RL_NPW; ++j)
#pragma unroll
    for (int g = 0; g < RL_G; ++g) acc[j][g] = 0.f;
  for (int seg = 0; seg < 2; ++seg) {
    const float* x = seg ? a.x2 : a.x1;
    const float* w = seg ? a.w2 : a.w1;
    const int K = seg ? a.K2 : a.K1, ldx = seg ? a.ldx2 : a.ldx1;
    if (x == nullptr || K == 0) continue;  // (uniform over the grid)
    for (int c0 = 0; c0 < K; c0 += RL_KC) {
      const int len = K - c0 < RL_KC ? K - c0 : RL_KC;
      __syncthreads();  // the previous chunk has been consumed
      rl_stage(xs, x, ldx, c0, len, r0, a.R, seg ? a.x2_zero : nullptr, NR);
      __syncthreads();
#pragma unroll
      for (int j = 0; j < RL_NPW; ++j)
        if (n0 + j < a.N) rl_dot<NR>(w + (long)(n0 + j) * K + c0, xs, len, lane, acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < RL_NPW; ++j) {
    const int n = n0 + j;
    if (n >= a.N) continue;  // (uniform over the wave)
    float mine = 0.f;
#pragma unroll
    for (int g = 0; g < NR; ++g) {
      const float s = wave_sum(acc[j][g]);  // xor butterfly 32, 16, .. 1: the same tree in every lane
      mine = lane == g ? s : mine;
    }
    if (lane < NR && r0 + lane < a.R) {
      float z = mine + a.b1[n];
      if (a.b2 != nullptr) z += a.b2[n];
      a.y[(long)(r0 + lane) * a.ldy + n] = act_apply(a.act, z);
    }
  }
}

__global__ __launch_bounds__(RL_WAVES * 64) void rows_linear2_kernel(RowsLinearArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[RL_G * RL_KC];
  const int left = a.R - blockIdx.y * RL_G;
  if (left <= 1) rows_linear2_body<1>(a, xs);
  else if (left <= 2) rows_linear2_body<2>(a, xs);
  else if (left <= 4) rows_linear2_body<4>(a, xs);
  else rows_linear2_body<8>(a, xs);
}

inline bool overlaps(const float* a, long na, const float* b, long nb) {
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + 4 * (uintptr_t)na, b0 = (uintptr_t)b, b1 = b0 + 4 * (uintptr_t)nb;
  return a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" int tacorl_rows_linear2_group(void) { return RL_G; }

extern "C" int tacorl_rows_linear2_supported(int R, int K1, int K2, int N) {
  return R >= 1 && R <= 64 && K1 >= 1 && K1 <= RL_MAX_DIM && K2 >= 0 && K2 <= RL_MAX_DIM && N >= 1 && N <= RL_MAX_DIM;
}

extern "C" int tacorl_rows_linear2_fwd(const float* x1, int ldx1, int K1, const float* w1, const float* b1, const float* x2,
                                       int ldx2, int K2, const float* w2, const float* b2,
                                       const unsigned char* x2_row_is_zero, float* y, int ldy, int R, int N, int act,
                                       tacorl_stream_t stream) {
  if (!tacorl_rows_linear2_supported(R, K1, K2, N)) return TACORL_EINVAL;
  if (!x1 || !w1 || !b1 || !y || ldx1 < K1 || ldy < N || act < ACT_NONE || act > ACT_TANH) return TACORL_EINVAL;
  if (x2 == nullptr) K2 = 0;  // a plain projection: w2 and the flags are not looked at (b2, if given, is still added)
  if (K2 > 0 && (!w2 || ldx2 < K2)) return TACORL_EINVAL;
  const uintptr_t al = (uintptr_t)x1 | (uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)y | (uintptr_t)x2 | (uintptr_t)w2 | (uintptr_t)b2;
  if (al & 3) return TACORL_EINVAL;
  const long ny = (long)(R - 1) * ldy + N;
  if (overlaps(y, ny, x1, (long)(R - 1) * ldx1 + K1)) return TACORL_EINVAL;
  if (K2 > 0 && overlaps(y, ny, x2, (long)(R - 1) * ldx2 + K2)) return TACORL_EINVAL;
  RowsLinearArgs a{x1, w1, b1, K2 > 0 ? x2 : nullptr, w2, b2, K2 > 0 ? x2_row_is_zero : nullptr, y,
                   ldx1, K1, ldx2, K2, ldy, R, N, act};
  hipLaunchKernelGGL(rows_linear2_kernel, dim3((unsigned)cdiv(N, RL_NPB), (unsigned)cdiv(R, RL_G)), dim3(RL_WAVES * 64), 0,
                     (hipStream_t)stream, a);
  return LAUNCH_OK();
}
