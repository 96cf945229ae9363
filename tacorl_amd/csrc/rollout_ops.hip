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
//
// tacorl_rows_mlp_fwd runs a whole MLP chain on this kernel in one host call - one launch per hidden layer on the caller's
// stream, the outputs kept in the caller's workspace - and ends it with an ordinary layer or with rows_policy_action_kernel,
// the deterministic action of a policy head.  Layers are separate launches: no cooperative launch, no grid barrier, no flag
// between workgroups.
#include "../../include/tacorl_hip.h"
#include "common.h"

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? TACORL_OK : TACORL_ELAUNCH)

namespace {

constexpr int RL_G = 8;        // rows per group (tacorl_rows_linear2_group)
constexpr int RL_KC = 2048;    // columns of [x1 | x2] staged at a time
constexpr int RL_WAVES = 4;    // waves per workgroup
constexpr int RL_NPW = 2;      // neurons per wave (tacorl_rows_linear2_fwd; tacorl_rows_mlp_fwd chooses per call)
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

template <int NR, int NPW>
__device__ __forceinline__ void rows_linear2_body(const RowsLinearArgs& a, float* xs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.y * RL_G;
  const int n0 = (blockIdx.x * RL_WAVES + wave) * NPW;
  float acc[NPW][RL_G];
#pragma unroll
  for (int j = 0; j < NPW; ++j)
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
      for (int j = 0; j < NPW; ++j)
        if (n0 + j < a.N) rl_dot<NR>(w + (long)(n0 + j) * K + c0, xs, len, lane, acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < NPW; ++j) {
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

// NPW neurons per wave, one after the other: a neuron's summation order does not depend on it (rl_dot per neuron), so every
// instantiation gives the same bits
template <int NPW>
__global__ __launch_bounds__(RL_WAVES * 64) void rows_linear2_kernel(RowsLinearArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[RL_G * RL_KC];
  const int left = a.R - blockIdx.y * RL_G;
  if (left <= 1) rows_linear2_body<1, NPW>(a, xs);
  else if (left <= 2) rows_linear2_body<2, NPW>(a, xs);
  else if (left <= 4) rows_linear2_body<4, NPW>(a, xs);
  else rows_linear2_body<8, NPW>(a, xs);
}

template <int NPW>
inline void rows_linear2_launch(const RowsLinearArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(rows_linear2_kernel<NPW>, dim3((unsigned)cdiv(a.N, RL_WAVES * NPW), (unsigned)cdiv(a.R, RL_G)),
                     dim3(RL_WAVES * 64), 0, stream, a);
}

// The last layer of a policy chain as the rollout reads it (reference actor.py:71-81, 99-104, deterministic): from the head
// matrix [fc_mean (Ac) | fc_log_std (Ac) | gripper_action (2)] only the Ac mean rows and - with dg - the two gripper rows are
// read; the log-std rows never are.  y[r] = [tanh(mean_0) .. tanh(mean_{Ac-1}) | +1 where logit_1 > logit_0, else -1]: a tie
// goes to -1, as torch.argmax picks index 0.  One wave per unit - a mean neuron, or the gripper pair (both logits in the same
// wave, one after the other, so the decision needs no second workgroup, no atomics and no second launch); staging, dot
// product and butterfly are those of rows_linear2_kernel, so a row's bits depend on its own inputs only.
// The reference clamps the mean to +-9 before the tanh: tanh(9) lies within one fp32 ulp of 1, below what any check of an
// fp32 tanh can resolve; the clamp is kept, it costs two instructions.
struct RowsPolicyArgs {
  const float *x, *w, *b;
  float* y;
  int ldx, K, ldy, R, Ac, dg;
};

template <int NR>
__device__ __forceinline__ void rows_policy_body(const RowsPolicyArgs& a, float* xs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.y * RL_G;
  const int u = blockIdx.x * RL_WAVES + wave;  // (uniform over the wave)
  const bool live = u < a.Ac + a.dg, grip = a.dg != 0 && u == a.Ac;
  const int n0 = grip ? 2 * a.Ac : u, n1 = 2 * a.Ac + 1;
  float acc0[RL_G], acc1[RL_G];
#pragma unroll
  for (int g = 0; g < RL_G; ++g) acc0[g] = acc1[g] = 0.f;
  for (int c0 = 0; c0 < a.K; c0 += RL_KC) {
    const int len = a.K - c0 < RL_KC ? a.K - c0 : RL_KC;
    __syncthreads();  // the previous chunk has been consumed
    rl_stage(xs, a.x, a.ldx, c0, len, r0, a.R, nullptr, NR);
    __syncthreads();
    if (live) rl_dot<NR>(a.w + (long)n0 * a.K + c0, xs, len, lane, acc0);
    if (grip) rl_dot<NR>(a.w + (long)n1 * a.K + c0, xs, len, lane, acc1);
  }
  if (!live) return;
  float m0 = 0.f, m1 = 0.f;
#pragma unroll
  for (int g = 0; g < NR; ++g) {
    const float s = wave_sum(acc0[g]);
    m0 = lane == g ? s : m0;
  }
  if (grip) {
#pragma unroll
    for (int g = 0; g < NR; ++g) {
      const float s = wave_sum(acc1[g]);
      m1 = lane == g ? s : m1;
    }
  }
  if (lane < NR && r0 + lane < a.R) {
    float* yr = a.y + (long)(r0 + lane) * a.ldy;
    const float z0 = m0 + a.b[n0];
    if (grip) {
      const float z1 = m1 + a.b[n1];
      yr[a.Ac] = z1 > z0 ? 1.f : -1.f;
    } else {
      yr[u] = tanhf(fminf(fmaxf(z0, -9.f), 9.f));
    }
  }
}

__global__ __launch_bounds__(RL_WAVES * 64) void rows_policy_action_kernel(RowsPolicyArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[RL_G * RL_KC];
  const int left = a.R - blockIdx.y * RL_G;
  if (left <= 1) rows_policy_body<1>(a, xs);
  else if (left <= 2) rows_policy_body<2>(a, xs);
  else if (left <= 4) rows_policy_body<4>(a, xs);
  else rows_policy_body<8>(a, xs);
}

constexpr int RM_MAX_LAYERS = 8;

// Neurons per wave of a chain layer of N neurons and R rows where the caller leaves the choice open.  Two neurons per wave
// give N / 8 workgroups per row group: 128 for a 1024-wide layer, half the GPU's 256 CUs.  Measured on the whole 4 x 1024
// low-level chain (profiles/ril_rollout.md, both arms): with one neuron per wave the chain takes 0.80 - 0.86 x the time at
// 1 .. 16 rows (one and two row groups: 128 and 256 workgroups at two neurons per wave) and 1.25 - 1.37 x from the third row
// group on, where twice the workgroups only stage the rows twice as often.  So: one neuron per wave where two would launch no more workgroups
// than the GPU has CUs.  Either form gives the same bits.
constexpr int RM_FILL_WGS = 256;
inline int rows_mlp_auto_npw(int N, int R) {
  return (long)cdiv(N, RL_WAVES * RL_NPW) * cdiv(R, RL_G) <= RM_FILL_WGS ? 1 : RL_NPW;
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
  rows_linear2_launch<RL_NPW>(a, (hipStream_t)stream);
  return LAUNCH_OK();
}

extern "C" int tacorl_rows_mlp_npw(int N, int R) { return rows_mlp_auto_npw(N, R); }

extern "C" int tacorl_rows_mlp_supported(int R, int n_layers, const int* dims, int mode, int Ac, int discrete_gripper) {
  if (R < 1 || R > 64 || n_layers < 1 || n_layers > RM_MAX_LAYERS || !dims) return 0;
  for (int l = 0; l <= n_layers; ++l)
    if (dims[l] < 1 || dims[l] > RL_MAX_DIM) return 0;
  if (mode == TACORL_ROWS_MLP_PLAIN) return 1;
  if (mode != TACORL_ROWS_MLP_POLICY_ACTION) return 0;
  return Ac >= 1 && Ac <= RL_MAX_DIM / 4 && dims[n_layers] >= 2 * Ac + (discrete_gripper ? 2 : 0);
}

extern "C" int tacorl_rows_mlp_fwd(const float* x, int ldx, int n_layers, const int* dims, const float* const* w,
                                   const float* const* b, const int* acts, float* ws, float* y, int ldy, int R, int mode,
                                   int Ac, int discrete_gripper, int npw, tacorl_stream_t stream) {
  const int dg = discrete_gripper ? 1 : 0;
  if (!tacorl_rows_mlp_supported(R, n_layers, dims, mode, Ac, dg)) return TACORL_EINVAL;
  if (!x || !w || !b || !acts || !y || (n_layers > 1 && !ws) || (npw != 0 && npw != 1 && npw != 2)) return TACORL_EINVAL;
  const bool policy = mode == TACORL_ROWS_MLP_POLICY_ACTION;
  const int ny = policy ? Ac + dg : dims[n_layers];
  if (ldx < dims[0] || ldy < ny) return TACORL_EINVAL;
  uintptr_t al = (uintptr_t)x | (uintptr_t)y | (uintptr_t)ws;
  long nws = 0;
  for (int l = 0; l < n_layers; ++l) {
    if (!w[l] || !b[l] || acts[l] < ACT_NONE || acts[l] > ACT_TANH) return TACORL_EINVAL;
    al |= (uintptr_t)w[l] | (uintptr_t)b[l];
    if (l + 1 < n_layers) nws += (long)R * dims[l + 1];
  }
  if (al & 3) return TACORL_EINVAL;
  const long nx = (long)(R - 1) * ldx + dims[0], nyy = (long)(R - 1) * ldy + ny;
  if (overlaps(y, nyy, x, nx) || (nws > 0 && (overlaps(ws, nws, x, nx) || overlaps(ws, nws, y, nyy)))) return TACORL_EINVAL;
  for (int l = 0; l < n_layers; ++l) {
    const long nw = (long)dims[l + 1] * dims[l];
    if (overlaps(y, nyy, w[l], nw) || overlaps(y, nyy, b[l], dims[l + 1])) return TACORL_EINVAL;
    if (nws > 0 && (overlaps(ws, nws, w[l], nw) || overlaps(ws, nws, b[l], dims[l + 1]))) return TACORL_EINVAL;
  }
  // every refusal is above: from here on only launches, on the caller's stream, each layer behind the one before it
  const float* in = x;
  int ldin = ldx;
  float* out = ws;
  for (int l = 0; l < n_layers; ++l) {
    const int K = dims[l], N = dims[l + 1];
    const bool last = l + 1 == n_layers;
    if (last && policy) {
      RowsPolicyArgs p{in, w[l], b[l], y, ldin, K, ldy, R, Ac, dg};
      hipLaunchKernelGGL(rows_policy_action_kernel, dim3((unsigned)cdiv(Ac + dg, RL_WAVES), (unsigned)cdiv(R, RL_G)),
                         dim3(RL_WAVES * 64), 0, (hipStream_t)stream, p);
    } else {
      RowsLinearArgs a{in, w[l], b[l], nullptr, nullptr, nullptr, nullptr, last ? y : out,
                       ldin, K, 0, 0, last ? ldy : N, R, N, acts[l]};
      // one neuron per wave where two would leave CUs without a workgroup (npw: 0 chooses, 1 / 2 force - the timing tool's arms)
      const int use = npw != 0 ? npw : rows_mlp_auto_npw(N, R);
      if (use == 1) rows_linear2_launch<1>(a, (hipStream_t)stream);
      else rows_linear2_launch<2>(a, (hipStream_t)stream);
    }
    if (hipGetLastError() != hipSuccess) return TACORL_ELAUNCH;
    in = out;
    ldin = N;
    out += (long)R * N;
  }
  return TACORL_OK;
}
