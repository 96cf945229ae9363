// Exact t-SNE of latent plans (the embedding behind the reference's TSNEPlot callback, utils/callbacks/tsne_plot.py; there it
// is MulticoreTSNE on host cores - a Barnes-Hut approximation with a sparse P, which this is NOT comparable with bit for bit).
// Definition: include/tacorl_hip.h "exact t-SNE"; fp64 restatement: tests/tsne_ref.py.
//
// Affinities (once per embedding):
//   tsne_normalise_kernel   one workgroup: column means, largest |x - mean|, the normalised table Xn [N][32] (zero padded) in ws
//   tsne_cond_kernel        one wave per row, 4 rows per workgroup: the row's N direct-form distances live in LDS; a bisection
//                           step is N / 64 LDS reads + expf per lane and one xor butterfly; writes p_{j|i} coalesced into P
//   tsne_symmetrise_kernel  in place: the workgroup of tile pair (a, b), a <= b, transposes both 64 x 64 tiles through LDS
//                           (rows padded to 65 floats: the column reads hit 64 different banks) and writes (c_ij + c_ji) / 2N
// One iteration (two launches, no host synchronisation, no atomics):
//   tsne_forces_kernel      one wave per row i: lane l owns the columns 4 l + 256 k .. + 3 (a 16-byte load of the P row where
//                           N % 4 == 0), y_j as float2 from global memory (all of Y is <= 64 KiB: L2), five fp32 accumulators,
//                           one butterfly.  A row's sums depend on that row of P and on Y only.
//   tsne_update_kernel      one workgroup: Z by a fixed tree, the gains / momentum update over the 2 N coordinates, the mean
//                           of the new Y by the same tree, the centring.
#include "../../include/tacorl_hip.h"
#include "common.h"

#include <math.h>
#include <stdint.h>

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? TACORL_OK : TACORL_ELAUNCH)

namespace {

constexpr int TSNE_MAX_N = 8192;  // the dense P is N^2 * 4 B = 256 MiB here, read once per iteration; distances 4 * 32 KiB of LDS
constexpr int TSNE_MAX_D = 32;
constexpr int TSNE_XP = 32;       // pitch of the normalised table
constexpr int TSNE_MAX_STEPS = 200;
constexpr int RED_T = 1024;       // the one-workgroup kernels
constexpr int SYM_TILE = 64;

struct WsLayout {
  size_t xn, attr, rep, zrow, krow, prow, scal, total;
};
inline WsLayout ws_layout(int N) {
  const size_t np = ((size_t)N + 3) & ~(size_t)3;
  WsLayout w;
  w.xn = 0;
  w.attr = w.xn + np * TSNE_XP * 4;
  w.rep = w.attr + np * 2 * 4;
  w.zrow = w.rep + np * 2 * 4;
  w.krow = w.zrow + np * 4;
  w.prow = w.krow + np * 4;
  w.scal = w.prow + np * 4;
  w.total = w.scal + 64;
  return w;
}

// Sum / max of one value per thread over the RED_T threads of the workgroup: shared-memory tree, stride halving
// (s[t] = s[t] + s[t + h], h = 512 .. 1).  Every thread returns the result.
__device__ __forceinline__ float block_sum(float v, float* s) {
  const int t = threadIdx.x;
  __syncthreads();
  s[t] = v;
  __syncthreads();
  for (int h = RED_T / 2; h > 0; h >>= 1) {
    if (t < h) s[t] = s[t] + s[t + h];
    __syncthreads();
  }
  return s[0];
}
__device__ __forceinline__ float block_max(float v, float* s) {
  const int t = threadIdx.x;
  __syncthreads();
  s[t] = v;
  __syncthreads();
  for (int h = RED_T / 2; h > 0; h >>= 1) {
    if (t < h) s[t] = fmaxf(s[t], s[t + h]);
    __syncthreads();
  }
  return s[0];
}

__global__ __launch_bounds__(RED_T) void tsne_normalise_kernel(const float* __restrict__ X, int N, int D, long ld,
                                                               float* __restrict__ xn, int* __restrict__ status) {
  __shared__ float red[RED_T];
  __shared__ float mean[TSNE_XP];
  const int t = threadIdx.x;
  for (int c = 0; c < D; ++c) {
    float acc = 0.f;
    for (int r = t; r < N; r += RED_T) acc = acc + X[(long)r * ld + c];
    const float s = block_sum(acc, red);
    if (t == 0) mean[c] = s / (float)N;
  }
  __syncthreads();
  float m = 0.f;
  for (int e = t; e < N * D; e += RED_T) {
    const int r = e / D, c = e - r * D;
    m = fmaxf(m, fabsf(X[(long)r * ld + c] - mean[c]));
  }
  const float big = block_max(m, red);
  for (int e = t; e < N * TSNE_XP; e += RED_T) {
    const int r = e / TSNE_XP, c = e % TSNE_XP;
    float v = 0.f;
    if (c < D && big > 0.f) v = (X[(long)r * ld + c] - mean[c]) / big;
    xn[e] = v;
  }
  if (t == 0) {
    status[0] = 0;                     // rows whose search ends at the step cap: counted by tsne_cond_kernel
    status[1] = big > 0.f ? 0 : 1;     // an all-equal table
  }
}

__global__ __launch_bounds__(256) void tsne_cond_kernel(const float* __restrict__ xn, int N, float logperp, float* __restrict__ P,
                                                        float* __restrict__ beta_out, int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) float tsne_dist[];  // [4][N]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + w;
  if (i >= N) return;  // (whole waves; no workgroup barrier below)
  float* dist = tsne_dist + (size_t)w * N;
  float q[TSNE_XP];
#pragma unroll
  for (int c = 0; c < TSNE_XP; c += 4) {
    const float4 v = *reinterpret_cast<const float4*>(xn + (size_t)i * TSNE_XP + c);
    q[c] = v.x; q[c + 1] = v.y; q[c + 2] = v.z; q[c + 3] = v.w;
  }
  float dmin = __int_as_float(0x7f800000);
  for (int j = lane; j < N; j += 64) {
    const float* p = xn + (size_t)j * TSNE_XP;
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < TSNE_XP; c += 4) {
      const float4 v = *reinterpret_cast<const float4*>(p + c);
      float t;
      t = q[c + 0] - v.x; acc = acc + t * t;
      t = q[c + 1] - v.y; acc = acc + t * t;
      t = q[c + 2] - v.z; acc = acc + t * t;
      t = q[c + 3] - v.w; acc = acc + t * t;
    }
    dist[j] = acc;
    if (j != i) dmin = fminf(dmin, acc);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) dmin = fminf(dmin, __shfl_xor(dmin, o, 64));
  // (each lane reads back only what it wrote itself: no barrier needed between the loops)

  float beta = 1.f, lo = 0.f, hi = 0.f, S = 1.f;
  bool have_lo = false, have_hi = false, capped = false;
  for (int step = 0;; ++step) {
    float s = 0.f, ws = 0.f;
    for (int j = lane; j < N; j += 64) {
      if (j == i) continue;
      const float t = dist[j] - dmin;
      const float e = expf(-(beta * t));
      s = s + e;
      ws = ws + e * t;
    }
    s = wave_sum(s);
    ws = wave_sum(ws);
    S = s;
    const float H = logf(s) + beta * ws / s;
    const float diff = H - logperp;
    if (fabsf(diff) < 1e-5f) break;
    if (step == TSNE_MAX_STEPS - 1) {
      capped = true;
      break;
    }
    if (diff > 0.f) {
      lo = beta, have_lo = true;
      beta = have_hi ? (beta + hi) / 2.f : fminf(beta * 2.f, 1e30f);
    } else {
      hi = beta, have_hi = true;
      beta = have_lo ? (beta + lo) / 2.f : beta / 2.f;
    }
  }
  for (int j = lane; j < N; j += 64) {
    const float t = dist[j] - dmin;
    P[(size_t)i * N + j] = j == i ? 0.f : expf(-(beta * t)) / S;
  }
  if (lane == 0) {
    beta_out[i] = beta;
    if (capped) atomicAdd(status, 1);  // an integer count: order-independent
  }
}

__global__ __launch_bounds__(256) void tsne_symmetrise_kernel(float* __restrict__ P, int N) {
  const int a = blockIdx.y, b = blockIdx.x;
  if (a > b) return;
  __shared__ float ta[SYM_TILE][SYM_TILE + 1];
  __shared__ float tb[SYM_TILE][SYM_TILE + 1];
  const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
  const float two_n = 2.f * (float)N;
  for (int r = r0; r < SYM_TILE; r += 4) {
    const int ra = a * SYM_TILE + r, ca = b * SYM_TILE + c;  // tile (a, b)
    const int rb = b * SYM_TILE + r, cb = a * SYM_TILE + c;  // tile (b, a)
    ta[r][c] = (ra < N && ca < N) ? P[(size_t)ra * N + ca] : 0.f;
    tb[r][c] = (rb < N && cb < N) ? P[(size_t)rb * N + cb] : 0.f;
  }
  __syncthreads();
  for (int r = r0; r < SYM_TILE; r += 4) {
    const int ra = a * SYM_TILE + r, ca = b * SYM_TILE + c;
    const int rb = b * SYM_TILE + r, cb = a * SYM_TILE + c;
    if (ra < N && ca < N) P[(size_t)ra * N + ca] = (ta[r][c] + tb[c][r]) / two_n;
    if (a != b && rb < N && cb < N) P[(size_t)rb * N + cb] = (tb[r][c] + ta[c][r]) / two_n;
  }
}

// MODE 0: the forces (attr, rep, Z_i).  MODE 1: the cost's row sums (sum_j P log P + P log(1 + q), sum_j P, Z_i).
template <int MODE>
__global__ __launch_bounds__(256) void tsne_rows_kernel(const float* __restrict__ P, const float* __restrict__ Y, int N,
                                                        float* __restrict__ o_a, float* __restrict__ o_b,
                                                        float* __restrict__ o_z) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const float2 yi = reinterpret_cast<const float2*>(Y)[i];
  const float* prow = P + (size_t)i * N;
  const bool vec = (N & 3) == 0;  // then every row base is 16-byte aligned and no group of four straddles the row end
  float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f, z = 0.f;
  for (int base = 4 * lane; base < N; base += 256) {
    float p[4];
    if (vec) {
      const float4 v = *reinterpret_cast<const float4*>(prow + base);
      p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) p[k] = base + k < N ? prow[base + k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = base + k;
      if (j >= N || j == i) continue;
      const float2 yj = reinterpret_cast<const float2*>(Y)[j];
      const float dx = yi.x - yj.x, dy = yi.y - yj.y;
      const float q = dx * dx + dy * dy;
      const float wgt = 1.f / (1.f + q);
      z = z + wgt;
      if (MODE == 0) {
        const float pw = p[k] * wgt, w2 = wgt * wgt;
        a0 = a0 + pw * dx;
        a1 = a1 + pw * dy;
        b0 = b0 + w2 * dx;
        b1 = b1 + w2 * dy;
      } else if (p[k] > 0.f) {
        a0 = a0 + p[k] * (logf(p[k]) + logf(1.f + q));
        b0 = b0 + p[k];
      }
    }
  }
  a0 = wave_sum(a0);
  b0 = wave_sum(b0);
  z = wave_sum(z);
  if (MODE == 0) {
    a1 = wave_sum(a1);
    b1 = wave_sum(b1);
  }
  if (lane == 0) {
    if (MODE == 0) {
      o_a[2 * i] = a0, o_a[2 * i + 1] = a1;
      o_b[2 * i] = b0, o_b[2 * i + 1] = b1;
    } else {
      o_a[i] = a0, o_b[i] = b0;
    }
    o_z[i] = z;
  }
}

__global__ __launch_bounds__(RED_T) void tsne_update_kernel(int N, float* __restrict__ Y, float* __restrict__ U,
                                                            float* __restrict__ G, const float* __restrict__ attr,
                                                            const float* __restrict__ rep, const float* __restrict__ zrow,
                                                            float ex, float mom, float lr, float* __restrict__ scal) {
  __shared__ float red[RED_T];
  const int t = threadIdx.x;
  float acc = 0.f;
  for (int r = t; r < N; r += RED_T) acc = acc + zrow[r];
  const float Z = block_sum(acc, red);
  float sx = 0.f, sy = 0.f;
  for (int r = t; r < N; r += RED_T) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int e = 2 * r + c;
      const float g = 4.f * (ex * attr[e] - rep[e] / Z);
      const float u = U[e];
      float gain = G[e];
      gain = ((g > 0.f) != (u > 0.f)) ? gain + 0.2f : gain * 0.8f;
      gain = fmaxf(gain, 0.01f);
      const float un = mom * u - lr * (gain * g);
      const float y = Y[e] + un;
      G[e] = gain, U[e] = un, Y[e] = y;
      if (c == 0) sx = sx + y; else sy = sy + y;
    }
  }
  const float mx = block_sum(sx, red) / (float)N;
  const float my = block_sum(sy, red) / (float)N;
  for (int r = t; r < N; r += RED_T) {  // (each thread re-reads only what it wrote itself)
    Y[2 * r] = Y[2 * r] - mx;
    Y[2 * r + 1] = Y[2 * r + 1] - my;
  }
  if (t == 0) scal[0] = Z;
}

__global__ __launch_bounds__(RED_T) void tsne_kl_finish_kernel(int N, const float* __restrict__ krow, const float* __restrict__ prow,
                                                               const float* __restrict__ zrow, float* __restrict__ out) {
  __shared__ float red[RED_T];
  const int t = threadIdx.x;
  float k = 0.f, p = 0.f, z = 0.f;
  for (int r = t; r < N; r += RED_T) k = k + krow[r], p = p + prow[r], z = z + zrow[r];
  k = block_sum(k, red);
  p = block_sum(p, red);
  z = block_sum(z, red);
  if (t == 0) out[0] = k + p * logf(z);
}

inline bool bad_ptr(const void* p, uintptr_t mask) { return !p || ((uintptr_t)p & mask); }

}  // namespace

extern "C" int tacorl_tsne_max_n(void) { return TSNE_MAX_N; }
extern "C" int tacorl_tsne_supported(long N, int D) { return N >= 4 && N <= TSNE_MAX_N && D >= 1 && D <= TSNE_MAX_D; }
extern "C" size_t tacorl_tsne_workspace_bytes(long N) { return N >= 4 && N <= TSNE_MAX_N ? ws_layout((int)N).total : 0; }

extern "C" int tacorl_tsne_workspace_offsets(long N, long* off) {
  if (N < 4 || N > TSNE_MAX_N || !off) return TACORL_EINVAL;
  const WsLayout w = ws_layout((int)N);
  off[0] = (long)w.xn, off[1] = (long)w.attr, off[2] = (long)w.rep, off[3] = (long)w.zrow;
  return TACORL_OK;
}

extern "C" int tacorl_tsne_affinities(const float* X, long N, int D, long ld, float perplexity, float* P, float* beta,
                                      int* status, void* ws, size_t ws_bytes, tacorl_stream_t stream) {
  if (!tacorl_tsne_supported(N, D) || ld < D || !(perplexity >= 1.f) || !(3.f * perplexity <= (float)(N - 1)))
    return TACORL_EINVAL;
  if (bad_ptr(X, 3) || bad_ptr(P, 15) || bad_ptr(beta, 3) || bad_ptr(status, 3) || bad_ptr(ws, 15) ||
      ws_bytes < tacorl_tsne_workspace_bytes(N))
    return TACORL_EINVAL;
  const int n = (int)N;
  const size_t lds = (size_t)4 * n * sizeof(float);
  static int attr = hipFuncSetAttribute(reinterpret_cast<const void*>(tsne_cond_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        4 * TSNE_MAX_N * (int)sizeof(float)) == hipSuccess ? 0 : -1;
  if (attr != 0) return TACORL_ELAUNCH;
  const hipStream_t st = (hipStream_t)stream;
  const WsLayout w = ws_layout(n);
  float* xn = reinterpret_cast<float*>((char*)ws + w.xn);
  hipLaunchKernelGGL(tsne_normalise_kernel, dim3(1), dim3(RED_T), 0, st, X, n, D, ld, xn, status);
  hipLaunchKernelGGL(tsne_cond_kernel, dim3((n + 3) / 4), dim3(256), lds, st, xn, n, logf(perplexity), P, beta, status);
  const int nt = (n + SYM_TILE - 1) / SYM_TILE;
  hipLaunchKernelGGL(tsne_symmetrise_kernel, dim3(nt, nt), dim3(256), 0, st, P, n);
  return LAUNCH_OK();
}

extern "C" int tacorl_tsne_step(const float* P, long N, float* Y, float* u, float* gains, float exaggeration, float momentum,
                                float lr, void* ws, size_t ws_bytes, tacorl_stream_t stream) {
  if (N < 4 || N > TSNE_MAX_N || bad_ptr(P, 15) || bad_ptr(Y, 7) || bad_ptr(u, 3) || bad_ptr(gains, 3) || bad_ptr(ws, 15) ||
      ws_bytes < tacorl_tsne_workspace_bytes(N))
    return TACORL_EINVAL;
  const int n = (int)N;
  const hipStream_t st = (hipStream_t)stream;
  const WsLayout w = ws_layout(n);
  char* b = (char*)ws;
  float *attr = (float*)(b + w.attr), *rep = (float*)(b + w.rep), *zrow = (float*)(b + w.zrow), *scal = (float*)(b + w.scal);
  hipLaunchKernelGGL(tsne_rows_kernel<0>, dim3((n + 3) / 4), dim3(256), 0, st, P, Y, n, attr, rep, zrow);
  hipLaunchKernelGGL(tsne_update_kernel, dim3(1), dim3(RED_T), 0, st, n, Y, u, gains, attr, rep, zrow, exaggeration, momentum, lr,
                     scal);
  return LAUNCH_OK();
}

extern "C" int tacorl_tsne_kl(const float* P, const float* Y, long N, float* out, void* ws, size_t ws_bytes,
                              tacorl_stream_t stream) {
  if (N < 4 || N > TSNE_MAX_N || bad_ptr(P, 15) || bad_ptr(Y, 7) || bad_ptr(out, 3) || bad_ptr(ws, 15) ||
      ws_bytes < tacorl_tsne_workspace_bytes(N))
    return TACORL_EINVAL;
  const int n = (int)N;
  const hipStream_t st = (hipStream_t)stream;
  const WsLayout w = ws_layout(n);
  char* b = (char*)ws;
  float *krow = (float*)(b + w.krow), *prow = (float*)(b + w.prow), *zrow = (float*)(b + w.zrow);
  hipLaunchKernelGGL(tsne_rows_kernel<1>, dim3((n + 3) / 4), dim3(256), 0, st, P, Y, n, krow, prow, zrow);
  hipLaunchKernelGGL(tsne_kl_finish_kernel, dim3(1), dim3(RED_T), 0, st, n, krow, prow, zrow, out);
  return LAUNCH_OK();
}
