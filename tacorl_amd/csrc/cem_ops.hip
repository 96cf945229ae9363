// Cross-entropy-method refinement of an action (or a latent plan) against the critics, one launch for the whole refinement
// (reference modules/cem/cem.py:69-104, used by evaluation/rollout_manager.py:99-136 and :331-369).
//
// The observation does not change during a refinement, so the caller encodes it once and hands over the embedding; the
// reference's per-iteration work (sample, evaluate Q on the population, argsort, refit, .item()) is a loop INSIDE the
// kernel.  One workgroup (4 waves) per problem row - R evaluation environments are R independent workgroups:
//   once      base_n[j] = b0[j] + sum_e W0[j][e] s_n[e]                      (observation part of Q layer 0, per net)
//   per iteration
//     population  a_r = clamp(mean + std * eps_r, -1, 1), gripper dimension snapped to +-1          (LDS, fp32)
//     per 64 rows, per net:  h0 = silu(base + W0[:, E:] a_r)  (K = A, FMA)  ->  hidden layers (MFMA, activations stay
//                            in LDS, weights stream from L2 as the B fragments)  ->  q_r = w_out . h + b_out
//                            (folded into the last hidden layer's epilogue; twin nets: min)
//     elites      rank count over the N fp32 Q values in LDS (ties: lower index first; NaN ranks last)
//     refit       mean / unbiased std over the elites, blended with alpha, std clamped; best-so-far action (strict >)
// Two compute modes as everywhere in the library: TACORL_F32 runs v_mfma_f32_16x16x4_f32 on the fp32 master weights (exact
// fp32 products and sums), TACORL_BF16 v_mfma_f32_16x16x32_bf16 on the block's bf16 mirror with activations rounded to bf16
// and fp32 accumulation.  Population, Q values, selection and statistics are fp32 in both.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/tacorl_hip.h"
#include "common.h"

#define CEM_H 256     // hidden width
#define CEM_RC 64     // population rows per pass through the network
#define CEM_MAXN 256  // population (one thread per candidate in the rank count)
#define CEM_AP 32     // action columns kept in LDS (zero padded): A <= 32
#define CEM_MAXE 256
#define CEM_MAXL 4    // hidden layers

struct CemArgs {
  const float* s[2];     // [R][E] embedding per net
  const float* p32[2];   // fp32 head block per net (tacorl_mlp_param_layout of [E + A, 256 x L, 1])
  const void* p16[2];    // its bf16 mirror (TACORL_BF16)
  const float* mean0;    // [R][A] or NULL (zeros)
  const float* eps;      // [R][iters][N][A]
  float* out;            // [R][A]
  float* ws;             // [R][1 + 2 A]: best Q, final mean, final std
  float *t_pop, *t_q, *t_mean, *t_std;  // optional trace
  int* t_elite;
  long woff[CEM_MAXL + 1], boff[CEM_MAXL + 1];
  int nnet, N, A, E, L, iters, n_elite, dg;
  float min_std, max_std, alpha;
};

template <typename Atom>
struct CemFrag;
template <>
struct CemFrag<AtomF32> {  // 4 consecutive k per lane, four 16x16x4 steps: step s multiplies k = 16 kb + 4 (lane >> 4) + s
  static __device__ __forceinline__ f32x4 ldg(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
  static __device__ __forceinline__ f32x4 mma(f32x4 a, f32x4 b, f32x4 c) {
#pragma unroll
    for (int s = 0; s < 4; s++) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], c, 0, 0, 0);
    return c;
  }
};
template <>
struct CemFrag<AtomBF16> {  // 8 consecutive k per lane, one 16x16x32 step.  The mirror is 8-byte aligned only.
  static __device__ __forceinline__ f32x4 ldg(const __bf16* p) {
    const f32x2 lo = *reinterpret_cast<const f32x2*>(p), hi = *reinterpret_cast<const f32x2*>(p + 4);
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
  }
  static __device__ __forceinline__ f32x4 mma(f32x4 a, f32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};

template <typename Atom>
__global__ __launch_bounds__(256) void cem_refine_kernel(const CemArgs a) {
  typedef typename Atom::elem elem;
  constexpr int EPL = 16 / sizeof(elem);  // elements per lane and fragment (16 bytes)
  constexpr int KB = 4 * EPL;             // k per fragment block
  constexpr int NKB = CEM_H / KB;
  constexpr int LDX = CEM_H + EPL;        // LDS row stride of the activations (16-byte pad)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  elem* X = reinterpret_cast<elem*>(smem);                                          // [CEM_RC][LDX]
  float* pop = reinterpret_cast<float*>(smem + sizeof(elem) * CEM_RC * LDX);       // [N][CEM_AP]
  float* qrow = pop + a.N * CEM_AP;                                                 // [N]
  float* qpart = qrow + CEM_MAXN;                                                   // [4][CEM_RC]
  float* base = qpart + 4 * CEM_RC;                                                 // [2][CEM_H]
  float* mean = base + 2 * CEM_H;                                                   // [CEM_AP]
  float* sd = mean + CEM_AP;                                                        // [CEM_AP]
  int* elite = reinterpret_cast<int*>(sd + CEM_AP);                                 // [N]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  const int row = blockIdx.x, N = a.N, A = a.A, E = a.E, K0 = a.E + a.A;
  const elem* P[2];
  for (int n = 0; n < 2; n++) P[n] = sizeof(elem) == 2 ? reinterpret_cast<const elem*>(a.p16[n]) : reinterpret_cast<const elem*>(a.p32[n]);

  // ---- once: the observation part of layer 0 (thread j = hidden unit j), the starting distribution
  for (int n = 0; n < a.nnet; n++) {
    const elem* w = P[n] + a.woff[0] + (long)tid * K0;
    const float* s = a.s[n] + (long)row * E;
    float z = a.p32[n][a.boff[0] + tid];
    for (int e = 0; e < E; e++) z = fmaf((float)w[e], (float)Atom::cvt(s[e]), z);
    base[n * CEM_H + tid] = z;
  }
  if (tid < CEM_AP) {
    mean[tid] = (tid < A && a.mean0) ? a.mean0[(long)row * A + tid] : 0.f;
    sd[tid] = a.max_std;
  }
  float best_q = -INFINITY, best_a = 0.f;  // threads < A: their own action dimension of the best elite so far
  __syncthreads();

  for (int it = 0; it < a.iters; it++) {
    // ---- population
    const long t0 = (long)row * a.iters + it;
    const float* eps = a.eps + t0 * N * A;
    for (int i = tid; i < N * CEM_AP; i += 256) {
      const int r = i / CEM_AP, d = i % CEM_AP;
      float v = 0.f;
      if (d < A) {
        v = mean[d] + eps[r * A + d] * sd[d];
        v = fminf(fmaxf(v, -1.f), 1.f);
        if (a.dg && d == A - 1) v = v >= 0.f ? 1.f : -1.f;
        if (a.t_pop) a.t_pop[(t0 * N + r) * A + d] = v;
      }
      pop[i] = v;
    }
    __syncthreads();

    // ---- Q of every candidate, CEM_RC rows at a time
    for (int r0 = 0; r0 < N; r0 += CEM_RC) {
      for (int n = 0; n < a.nnet; n++) {
        {  // layer 0: K = A on top of the observation part
          float w0[CEM_AP];
          const elem* w = P[n] + a.woff[0] + (long)tid * K0 + E;
#pragma unroll
          for (int d = 0; d < CEM_AP; d++) w0[d] = d < A ? (float)w[d] : 0.f;
          const float b = base[n * CEM_H + tid];
          for (int r = 0; r < CEM_RC; r++) {
            const f32x4* pr = reinterpret_cast<const f32x4*>(pop + (r0 + r) * CEM_AP);
            float z = b;
#pragma unroll
            for (int d4 = 0; d4 < CEM_AP / 4; d4++) {
              const f32x4 p = pr[d4];
#pragma unroll
              for (int u = 0; u < 4; u++) z = fmaf(w0[4 * d4 + u], (float)Atom::cvt(p[u]), z);
            }
            X[r * LDX + tid] = Atom::cvt(act_apply(ACT_SILU, z));
          }
        }
        __syncthreads();
        for (int l = 1; l < a.L; l++) {
          // wave w: output columns 64 w .. 64 w + 63 of all CEM_RC rows; acc[rt][ct]: rows 16 rt + 4 g + reg, column
          // 64 w + 16 ct + c
          f32x4 acc[4][4];
#pragma unroll
          for (int rt = 0; rt < 4; rt++)
#pragma unroll
            for (int ct = 0; ct < 4; ct++) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
          const elem* wp = P[n] + a.woff[l] + (long)(64 * wave + c) * CEM_H + EPL * g;
          const elem* xp = X + c * LDX + EPL * g;
          f32x4 b[4], bn[4];
#pragma unroll
          for (int ct = 0; ct < 4; ct++) b[ct] = CemFrag<Atom>::ldg(wp + (long)ct * 16 * CEM_H);
#pragma unroll 2
          for (int kb = 0; kb < NKB; kb++) {
            const int kn = kb + 1 < NKB ? kb + 1 : kb;  // (the last block re-reads itself: no branch around the loads)
#pragma unroll
            for (int ct = 0; ct < 4; ct++) bn[ct] = CemFrag<Atom>::ldg(wp + (long)ct * 16 * CEM_H + kn * KB);
            f32x4 av[4];
#pragma unroll
            for (int rt = 0; rt < 4; rt++) av[rt] = *reinterpret_cast<const f32x4*>(xp + rt * 16 * LDX + kb * KB);
#pragma unroll
            for (int rt = 0; rt < 4; rt++)
#pragma unroll
              for (int ct = 0; ct < 4; ct++) acc[rt][ct] = CemFrag<Atom>::mma(av[rt], b[ct], acc[rt][ct]);
#pragma unroll
            for (int ct = 0; ct < 4; ct++) b[ct] = bn[ct];
          }
          const float* bias = a.p32[n] + a.boff[l];
          if (l + 1 < a.L) {
            __syncthreads();  // every wave has read the layer's input: overwrite it in place
#pragma unroll
            for (int ct = 0; ct < 4; ct++) {
              const int col = 64 * wave + 16 * ct + c;
              const float bj = bias[col];
#pragma unroll
              for (int rt = 0; rt < 4; rt++)
#pragma unroll
                for (int q = 0; q < 4; q++)
                  X[(16 * rt + 4 * g + q) * LDX + col] = Atom::cvt(act_apply(ACT_SILU, acc[rt][ct][q] + bj));
            }
            __syncthreads();
          } else {
            // last hidden layer: the output layer's dot product in the epilogue
            float part[4][4];
#pragma unroll
            for (int rt = 0; rt < 4; rt++)
#pragma unroll
              for (int q = 0; q < 4; q++) part[rt][q] = 0.f;
#pragma unroll
            for (int ct = 0; ct < 4; ct++) {
              const int col = 64 * wave + 16 * ct + c;
              const float bj = bias[col], wo = (float)P[n][a.woff[a.L] + col];
#pragma unroll
              for (int rt = 0; rt < 4; rt++)
#pragma unroll
                for (int q = 0; q < 4; q++)
                  part[rt][q] = fmaf(wo, (float)Atom::cvt(act_apply(ACT_SILU, acc[rt][ct][q] + bj)), part[rt][q]);
            }
#pragma unroll
            for (int rt = 0; rt < 4; rt++)
#pragma unroll
              for (int q = 0; q < 4; q++) {
                const float v = row16_sum(part[rt][q]);
                if (c == 0) qpart[wave * CEM_RC + 16 * rt + 4 * g + q] = v;
              }
            __syncthreads();
            if (tid < CEM_RC) {
              float q = a.p32[n][a.boff[a.L]];
#pragma unroll
              for (int w = 0; w < 4; w++) q += qpart[w * CEM_RC + tid];
              qrow[r0 + tid] = n == 0 ? q : fminf(qrow[r0 + tid], q);
            }
          }
        }
      }
    }
    __syncthreads();

    // ---- elites: rank k = the k-th largest Q (ties: lower index first).  A NaN ranks as -inf, so the ranks are a
    // permutation of 0 .. N-1 whatever the values are and every elite slot is written
    if (tid < N) {
      const float qi = qrow[tid];
      const float ki = qi != qi ? -INFINITY : qi;
      int rank = 0;
      for (int j = 0; j < N; j++) {
        float kj = qrow[j];
        kj = kj != kj ? -INFINITY : kj;
        rank += (kj > ki || (kj == ki && j < tid)) ? 1 : 0;
      }
      if (rank < a.n_elite) {
        elite[rank] = tid;
        if (a.t_elite) a.t_elite[t0 * a.n_elite + rank] = tid;
      }
      if (a.t_q) a.t_q[t0 * N + tid] = qi;
    }
    __syncthreads();

    // ---- refit (thread d = action dimension d)
    if (tid < A) {
      const int ne = a.n_elite;
      float m = 0.f;
      for (int k = 0; k < ne; k++) m += pop[elite[k] * CEM_AP + tid];
      m /= (float)ne;
      float v = 0.f;
      for (int k = 0; k < ne; k++) {
        const float d = pop[elite[k] * CEM_AP + tid] - m;
        v = fmaf(d, d, v);
      }
      const float s = sqrtf(v / (float)(ne - 1));
      const float nm = a.alpha * mean[tid] + (1.f - a.alpha) * m;
      float ns = a.alpha * sd[tid] + (1.f - a.alpha) * s;
      ns = fminf(fmaxf(ns, a.min_std), a.max_std);
      const float qb = qrow[elite[0]];
      if (qb > best_q) {
        best_q = qb;
        best_a = pop[elite[0] * CEM_AP + tid];
      }
      mean[tid] = nm;
      sd[tid] = ns;
      if (a.t_mean) a.t_mean[t0 * A + tid] = nm;
      if (a.t_std) a.t_std[t0 * A + tid] = ns;
    }
    __syncthreads();
  }
  if (tid < A) {
    a.out[(long)row * A + tid] = best_a;
    float* w = a.ws + (long)row * (1 + 2 * A);
    if (tid == 0) w[0] = best_q;
    w[1 + tid] = mean[tid];
    w[1 + A + tid] = sd[tid];
  }
}

static size_t cem_lds_bytes(int N, int compute) {
  const size_t es = compute == TACORL_BF16 ? 2 : 4;
  return es * CEM_RC * (CEM_H + 16 / es) + sizeof(float) * ((size_t)N * CEM_AP + CEM_MAXN + 4 * CEM_RC + 2 * CEM_H + 2 * CEM_AP) +
         sizeof(int) * (size_t)N;
}

extern "C" int tacorl_cem_supported(int N, int A, int E, int hidden, int q_layers, int compute) {
  return hidden == CEM_H && N >= CEM_RC && N <= CEM_MAXN && N % CEM_RC == 0 && A >= 1 && A <= CEM_AP && E >= 1 && E <= CEM_MAXE &&
         q_layers >= 2 && q_layers <= CEM_MAXL && (compute == TACORL_F32 || compute == TACORL_BF16);
}

extern "C" size_t tacorl_cem_ws_bytes(int R, int N, int A, int E, int hidden, int q_layers, int compute) {
  if (R < 1 || !tacorl_cem_supported(N, A, E, hidden, q_layers, compute)) return 0;
  return sizeof(float) * (size_t)R * (1 + 2 * A);
}

extern "C" int tacorl_cem_refine(int R, int nnet, const float* const* s, const float* const* params,
                                 const void* const* params_bf16, const float* mean0, const float* eps, float* out, int N,
                                 int A, int E, int hidden, int q_layers, int iters, int n_elite, float min_std, float max_std,
                                 float alpha, int discrete_gripper, int compute, float* t_pop, float* t_q, int* t_elite,
                                 float* t_mean, float* t_std, void* ws, size_t ws_bytes, tacorl_stream_t stream) {
  if (!tacorl_cem_supported(N, A, E, hidden, q_layers, compute)) return TACORL_EINVAL;
  if (R < 1 || R > 65535 || nnet < 1 || nnet > 2 || iters < 1 || n_elite < 2 || n_elite > N) return TACORL_EINVAL;
  if (!(min_std > 0.f) || !(max_std >= min_std) || !(alpha >= 0.f && alpha <= 1.f)) return TACORL_EINVAL;
  if (!s || !params || !eps || !out || !ws || ws_bytes < tacorl_cem_ws_bytes(R, N, A, E, hidden, q_layers, compute)) return TACORL_EINVAL;
  if (compute == TACORL_BF16 && !params_bf16) return TACORL_EINVAL;
  CemArgs a = {};
  for (int n = 0; n < nnet; n++) {
    if (!s[n] || !params[n] || ((uintptr_t)params[n] & 15)) return TACORL_EINVAL;
    if (compute == TACORL_BF16 && (!params_bf16[n] || ((uintptr_t)params_bf16[n] & 7))) return TACORL_EINVAL;
    a.s[n] = s[n];
    a.p32[n] = params[n];
    a.p16[n] = compute == TACORL_BF16 ? params_bf16[n] : nullptr;
  }
  int dims[CEM_MAXL + 2];
  dims[0] = E + A;
  for (int l = 1; l <= q_layers; l++) dims[l] = hidden;
  dims[q_layers + 1] = 1;
  tacorl_mlp_param_layout(q_layers + 1, dims, a.woff, a.boff);
  a.mean0 = mean0; a.eps = eps; a.out = out; a.ws = static_cast<float*>(ws);
  a.t_pop = t_pop; a.t_q = t_q; a.t_elite = t_elite; a.t_mean = t_mean; a.t_std = t_std;
  a.nnet = nnet; a.N = N; a.A = A; a.E = E; a.L = q_layers; a.iters = iters; a.n_elite = n_elite; a.dg = discrete_gripper ? 1 : 0;
  a.min_std = min_std; a.max_std = max_std; a.alpha = alpha;
  const int lds_max = (int)cem_lds_bytes(CEM_MAXN, TACORL_F32);
  static int once = (hipFuncSetAttribute(reinterpret_cast<const void*>(cem_refine_kernel<AtomF32>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) == hipSuccess &&
                     hipFuncSetAttribute(reinterpret_cast<const void*>(cem_refine_kernel<AtomBF16>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) == hipSuccess) ? 0 : -1;
  if (once != 0) return TACORL_ELAUNCH;
  const size_t lds = cem_lds_bytes(N, compute);
  if (compute == TACORL_BF16)
    hipLaunchKernelGGL(cem_refine_kernel<AtomBF16>, dim3(R), dim3(256), lds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(cem_refine_kernel<AtomF32>, dim3(R), dim3(256), lds, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? TACORL_OK : TACORL_ELAUNCH;
}
