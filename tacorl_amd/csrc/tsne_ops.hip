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

// ======================================================================================================================
// Neighbour-sparse t-SNE (include/tacorl_hip.h "neighbour-sparse t-SNE"; fp64 restatement: tests/tsne_nbr_ref.py): the
// reference library's sparse P over the K = floor(3 perplexity) nearest neighbours, exact repulsion (Barnes-Hut at theta = 0),
// nothing of size N x N.  Normalisation, update, centring and the cost's last step are the dense path's kernels above.
//
// Affinities (once per embedding):
//   tsne_normalise_kernel   (the dense one)
//   nbr_knn_kernel          tacorl_knn_l2's shape - one thread per query, the table through LDS in tiles of NBR_KNN_TILE rows,
//                           the sorted (d, row) lists in LDS slot-major - with lists of up to 192 entries (64 queries per
//                           workgroup: 96 KiB of lists) and the query's own row left out by index; a NaN distance counts
//                           as +inf, so a list is K valid rows whatever the table holds
//   nbr_cond_kernel         one wave per row: the K distances in registers (<= 3 per lane), the dense bisection
//   nbr_count / nbr_scan / nbr_fill / nbr_sort   the symmetric CSR: a row's length is K + the number of rows that list it
//                           without being listed back (an integer atomic count); row_ptr is their exclusive scan; the fill
//                           writes a row's own K entries and appends the one-sided in-entries at an atomic cursor; the sort
//                           (one workgroup per row, a same-direction bitonic network on (col, val), in LDS where the row fits
//                           and in place in global memory for a hub row) makes the columns ascend, so that nothing depends
//                           on the order in which the atomics landed
// One iteration (three launches, no host synchronisation, no float atomics):
//   nbr_rep_kernel          workgroup (b, s): thread t owns row i = 256 b + t and adds the j of segment s in ascending order,
//                           Y through LDS in tiles of 256 (a broadcast read); partial (rep, Z_i) per (segment, row)
//   nbr_rows_kernel         one wave per row: the stored entries (attr, or the cost's sums), then the segments' partials
//                           folded in ascending segment order
//   tsne_update_kernel      (the dense one)
namespace {

constexpr int NBR_MAX_N = 131072;
constexpr int NBR_MAX_K = 192;
constexpr int NBR_KNN_TILE = 128;   // database rows per LDS tile
constexpr int NBR_KNN_T = 64;       // queries per workgroup: lists of 64 * 192 * 8 B = 96 KiB, + 16 KiB of tile <= 160 KiB
constexpr int NBR_REP_T = 256;      // rows per repulsion workgroup = j per LDS tile
constexpr int NBR_MAX_SEG = 32;     // segments of the j range
constexpr int NBR_SORT_T = 256;
constexpr int NBR_SORT_LDS = 4096;  // row entries sorted in LDS (32 KiB); longer rows in place

// Segment length: the smallest multiple of 256 with at most 32 segments - 256 up to N = 8192, 4096 at 131072.
inline int nbr_segment(int N) { return NBR_REP_T * ((N + NBR_REP_T * NBR_MAX_SEG - 1) / (NBR_REP_T * NBR_MAX_SEG)); }

struct NbrWsLayout {
  size_t xn, attr, rep, zrow, krow, prow, scal, cnt, part, total;
};
inline NbrWsLayout nbr_ws_layout(int N) {
  const size_t np = ((size_t)N + 3) & ~(size_t)3;
  NbrWsLayout w;
  w.xn = 0;
  w.attr = w.xn + np * TSNE_XP * 4;
  w.rep = w.attr + np * 2 * 4;
  w.zrow = w.rep + np * 2 * 4;
  w.krow = w.zrow + np * 4;
  w.prow = w.krow + np * 4;
  w.scal = w.prow + np * 4;
  w.cnt = w.scal + 64;
  w.part = w.cnt + np * 4;
  const size_t S = (size_t)((N + nbr_segment(N) - 1) / nbr_segment(N));
  w.total = w.part + S * 3 * np * 4;
  return w;
}

template <int DP>
__global__ __launch_bounds__(NBR_KNN_T) void nbr_knn_kernel(const float* __restrict__ points, int n_points, int D, long ld, int k,
                                                            int* __restrict__ nbr_row, float* __restrict__ nbr_dist) {
  constexpr int T = NBR_KNN_T;
  extern __shared__ __attribute__((aligned(16))) unsigned char nbr_smem[];
  float* tile = reinterpret_cast<float*>(nbr_smem);           // [NBR_KNN_TILE][DP]
  float* ld_d = tile + NBR_KNN_TILE * DP;                     // [k][T]
  int* ld_r = reinterpret_cast<int*>(ld_d + (size_t)k * T);   // [k][T]
  const int tid = threadIdx.x;
  const int qi = blockIdx.x * T + tid;
  const bool live = qi < n_points;
  const int qrow = live ? qi : n_points - 1;                  // (idle threads of the last block mirror its last query)

  float q[DP];
#pragma unroll
  for (int j = 0; j < DP; ++j) q[j] = j < D ? points[(long)qrow * ld + j] : 0.f;
  for (int s = 0; s < k; ++s) {
    ld_d[s * T + tid] = __int_as_float(0x7f800000);
    ld_r[s * T + tid] = -1;
  }
  int thr = 0x7f800001;  // above the bits of +inf while the list has free slots

  constexpr int NPRE = NBR_KNN_TILE * DP / T;
  float pre[NPRE];
  auto fetch = [&](int base) {
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
      const int e = tid + i * T;
      const int r = base + e / DP, c = e % DP;
      pre[i] = (r < n_points && c < D) ? points[(long)r * ld + c] : 0.f;  // rows past the table are never read
    }
  };
  auto insert = [&](float d, int row) {
    int j = k - 1;
    while (j > 0) {
      const float pd = ld_d[(j - 1) * T + tid];
      const int pr = ld_r[(j - 1) * T + tid];
      if (pr >= 0 && !(pd > d)) break;  // an equal distance was found at a lower row: it stays in front
      ld_d[j * T + tid] = pd;
      ld_r[j * T + tid] = pr;
      --j;
    }
    ld_d[j * T + tid] = d;
    ld_r[j * T + tid] = row;
    thr = ld_r[(k - 1) * T + tid] >= 0 ? __float_as_int(ld_d[(k - 1) * T + tid]) : 0x7f800001;
  };
  auto dist = [&](const float* p) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < DP; c += 4) {
      const float4 v = *reinterpret_cast<const float4*>(p + c);
      float t;
      t = q[c + 0] - v.x; acc = acc + t * t;
      t = q[c + 1] - v.y; acc = acc + t * t;
      t = q[c + 2] - v.z; acc = acc + t * t;
      t = q[c + 3] - v.w; acc = acc + t * t;
    }
    return acc == acc ? acc : __int_as_float(0x7f800000);  // a NaN distance counts as +inf: it still fills a free slot
  };

  fetch(0);
  for (int base = 0; base < n_points; base += NBR_KNN_TILE) {
    __syncthreads();  // every thread is done with the previous tile
#pragma unroll
    for (int i = 0; i < NPRE; ++i) tile[tid + i * T] = pre[i];
    __syncthreads();
    if (base + NBR_KNN_TILE < n_points) fetch(base + NBR_KNN_TILE);
    const int valid = n_points - base < NBR_KNN_TILE ? n_points - base : NBR_KNN_TILE;
    int r = 0;
    for (; r + 4 <= valid; r += 4) {  // four independent accumulation chains
      const float d0 = dist(tile + (r + 0) * DP), d1 = dist(tile + (r + 1) * DP);
      const float d2 = dist(tile + (r + 2) * DP), d3 = dist(tile + (r + 3) * DP);
      if (__float_as_int(d0) < thr && base + r + 0 != qrow) insert(d0, base + r + 0);
      if (__float_as_int(d1) < thr && base + r + 1 != qrow) insert(d1, base + r + 1);
      if (__float_as_int(d2) < thr && base + r + 2 != qrow) insert(d2, base + r + 2);
      if (__float_as_int(d3) < thr && base + r + 3 != qrow) insert(d3, base + r + 3);
    }
    for (; r < valid; ++r) {
      const float d = dist(tile + r * DP);
      if (__float_as_int(d) < thr && base + r != qrow) insert(d, base + r);
    }
  }
  if (!live) return;
  for (int s = 0; s < k; ++s) {
    nbr_row[(size_t)qi * k + s] = ld_r[s * T + tid];
    nbr_dist[(size_t)qi * k + s] = ld_d[s * T + tid];
  }
}

template <int DP>
int nbr_knn_launch(const float* points, int n, int D, long ld, int k, int* nbr_row, float* nbr_dist, hipStream_t st) {
  constexpr int max_lds = NBR_KNN_TILE * DP * 4 + NBR_KNN_T * NBR_MAX_K * 8;
  static int attr = hipFuncSetAttribute(reinterpret_cast<const void*>(nbr_knn_kernel<DP>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        max_lds) == hipSuccess ? 0 : -1;
  if (attr != 0) return TACORL_ELAUNCH;
  const size_t lds = (size_t)NBR_KNN_TILE * DP * 4 + (size_t)NBR_KNN_T * k * 8;
  hipLaunchKernelGGL((nbr_knn_kernel<DP>), dim3((n + NBR_KNN_T - 1) / NBR_KNN_T), dim3(NBR_KNN_T), lds, st, points, n, D, ld, k,
                     nbr_row, nbr_dist);
  return LAUNCH_OK();
}

int nbr_knn_dispatch(const float* points, int n, int D, long ld, int k, int* nbr_row, float* nbr_dist, hipStream_t st) {
  // (zero padding of the columns adds +0 to a non-negative sum: the padded width changes no bit)
  if (D <= 4) return nbr_knn_launch<4>(points, n, D, ld, k, nbr_row, nbr_dist, st);
  if (D <= 8) return nbr_knn_launch<8>(points, n, D, ld, k, nbr_row, nbr_dist, st);
  if (D <= 16) return nbr_knn_launch<16>(points, n, D, ld, k, nbr_row, nbr_dist, st);
  return nbr_knn_launch<32>(points, n, D, ld, k, nbr_row, nbr_dist, st);
}

// One wave per row, list position s = lane + 64 c (c < 3) in registers.
__global__ __launch_bounds__(256) void nbr_cond_kernel(const float* __restrict__ nbr_dist, int N, int K, float logperp,
                                                       float* __restrict__ cond, float* __restrict__ beta_out,
                                                       int* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const float* drow = nbr_dist + (size_t)i * K;
  const float dmin = drow[0];
  float t[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) t[c] = lane + 64 * c < K ? drow[lane + 64 * c] - dmin : 0.f;
  float beta = 1.f, lo = 0.f, hi = 0.f, S = 1.f;
  bool have_lo = false, have_hi = false, capped = false;
  for (int step = 0;; ++step) {
    float s = 0.f, ws = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (lane + 64 * c < K) {
        const float e = expf(-(beta * t[c]));
        s = s + e;
        ws = ws + e * t[c];
      }
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
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (lane + 64 * c < K) cond[(size_t)i * K + lane + 64 * c] = expf(-(beta * t[c])) / S;
  if (lane == 0) {
    beta_out[i] = beta;
    if (capped) atomicAdd(status, 1);  // an integer count: order-independent
  }
}

// The list position of row i in row j's list, or -1: every lane of the wave returns it.
__device__ __forceinline__ int nbr_find(const int* __restrict__ nbr_row, int K, int j, int i, int lane) {
  const int* l = nbr_row + (size_t)j * K;
  int pos = -1;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int s = lane + 64 * c;
    if (s < K && l[s] == i) pos = s;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pos = max(pos, __shfl_xor(pos, o, 64));
  return pos;
}

__global__ __launch_bounds__(256) void nbr_zero_kernel(int* __restrict__ cnt, int N) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N) cnt[i] = 0;
}

__global__ __launch_bounds__(256) void nbr_count_kernel(const int* __restrict__ nbr_row, int N, int K, int* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  for (int s = 0; s < K; ++s) {
    const int j = nbr_row[(size_t)i * K + s];
    if ((unsigned)j >= (unsigned)N) continue;  // (never with this library's lists: every entry is a row)
    if (nbr_find(nbr_row, K, j, i, lane) < 0 && lane == 0) atomicAdd(cnt + j, 1);
  }
}

// row_ptr = exclusive scan of K + cnt; cnt is zeroed (it becomes the fill's cursor).  Thread t owns a contiguous chunk.
__global__ __launch_bounds__(RED_T) void nbr_scan_kernel(int N, int K, int* __restrict__ cnt, int* __restrict__ row_ptr) {
  __shared__ int part[RED_T];
  const int t = threadIdx.x;
  const int per = (N + RED_T - 1) / RED_T;
  const int a = min(t * per, N), b = min(a + per, N);
  int s = 0;
  for (int r = a; r < b; ++r) s += K + cnt[r];
  part[t] = s;
  __syncthreads();
  for (int h = 1; h < RED_T; h <<= 1) {  // Hillis-Steele, inclusive (integers: exact in any order)
    const int v = t >= h ? part[t - h] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - s;
  for (int r = a; r < b; ++r) {
    row_ptr[r] = run;
    run += K + cnt[r];
    cnt[r] = 0;
  }
  if (t == RED_T - 1) row_ptr[N] = part[t];
}

__global__ __launch_bounds__(256) void nbr_fill_kernel(const int* __restrict__ nbr_row, const float* __restrict__ cond, int N, int K,
                                                       const int* __restrict__ row_ptr, int* __restrict__ cursor,
                                                       int* __restrict__ col, float* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const float two_n = 2.f * (float)N;
  const int base = row_ptr[i];
  for (int s = 0; s < K; ++s) {
    const int j = nbr_row[(size_t)i * K + s];
    if ((unsigned)j >= (unsigned)N) continue;  // (as in the count: the row keeps an unwritten slot, nothing is addressed by j)
    const int back = nbr_find(nbr_row, K, j, i, lane);
    if (lane != 0) continue;
    const float a = cond[(size_t)i * K + s];                          // p_{j|i}
    const float b = back >= 0 ? cond[(size_t)j * K + back] : 0.f;     // p_{i|j}
    col[base + s] = j;
    val[base + s] = (a + b) / two_n;
    if (back < 0) {  // row j's entry at column i: (0 + p_{j|i}) / 2N
      const int e = row_ptr[j] + K + atomicAdd(cursor + j, 1);
      col[e] = i;
      val[e] = (0.f + a) / two_n;
    }
  }
}

// Same-direction bitonic network over n (col, val) pairs by col: positions >= n count as +inf and never move.
__device__ void nbr_sort_pairs(int* c, float* v, int n) {
  int m = 1;
  while (m < n) m <<= 1;
  for (int k = 2; k <= m; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int x = threadIdx.x; x < (m >> 1); x += NBR_SORT_T) {
        // pair number x: lower index lo, partner hi (the first step of a merge mirrors inside the block of k)
        const int lo = ((x / j) * 2 * j) + (x % j);
        const int hi = (j == (k >> 1)) ? ((lo / k) * k + k - 1 - (lo % k)) : lo + j;
        if (hi < n) {
          const int cl = c[lo], ch = c[hi];
          if (cl > ch) {
            const float vl = v[lo], vh = v[hi];
            c[lo] = ch, c[hi] = cl, v[lo] = vh, v[hi] = vl;
          }
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(NBR_SORT_T) void nbr_sort_kernel(const int* __restrict__ row_ptr, int* __restrict__ col,
                                                              float* __restrict__ val) {
  __shared__ int sc[NBR_SORT_LDS];
  __shared__ float sv[NBR_SORT_LDS];
  const int i = blockIdx.x;
  const int a = row_ptr[i], n = row_ptr[i + 1] - a;
  if (n <= NBR_SORT_LDS) {
    for (int x = threadIdx.x; x < n; x += NBR_SORT_T) sc[x] = col[a + x], sv[x] = val[a + x];
    __syncthreads();
    nbr_sort_pairs(sc, sv, n);
    for (int x = threadIdx.x; x < n; x += NBR_SORT_T) col[a + x] = sc[x], val[a + x] = sv[x];
  } else {
    nbr_sort_pairs(col + a, val + a, n);
  }
}

// Partial repulsion of (row block, segment): thread t adds the segment's j in ascending order.
__global__ __launch_bounds__(NBR_REP_T) void nbr_rep_kernel(const float* __restrict__ Y, int N, int seg_len, int np,
                                                            float* __restrict__ part) {
  __shared__ float2 ty[NBR_REP_T];
  const int t = threadIdx.x;
  const int i = blockIdx.x * NBR_REP_T + t;
  const int seg = blockIdx.y;
  const float2 yi = reinterpret_cast<const float2*>(Y)[i < N ? i : N - 1];
  const int j0 = seg * seg_len, j1 = min(j0 + seg_len, N);
  float b0 = 0.f, b1 = 0.f, z = 0.f;
  for (int base = j0; base < j1; base += NBR_REP_T) {
    __syncthreads();
    if (base + t < j1) ty[t] = reinterpret_cast<const float2*>(Y)[base + t];
    __syncthreads();
    const int valid = min(NBR_REP_T, j1 - base);
    for (int r = 0; r < valid; ++r) {
      const float2 yj = ty[r];
      const float dx = yi.x - yj.x, dy = yi.y - yj.y;
      const float q = dx * dx + dy * dy;
      const float wgt = base + r == i ? 0.f : 1.f / (1.f + q);  // (a zero term leaves the sums' bits as skipping it does)
      const float w2 = wgt * wgt;
      z = z + wgt;
      b0 = b0 + w2 * dx;
      b1 = b1 + w2 * dy;
    }
  }
  if (i < N) {
    float* p = part + (size_t)seg * 3 * np;
    p[i] = b0, p[np + i] = b1, p[2 * (size_t)np + i] = z;
  }
}

// MODE 0: attr over the row's stored entries.  MODE 1: the cost's row sums.  Both fold the segments' partials.
template <int MODE>
__global__ __launch_bounds__(256) void nbr_rows_kernel(const int* __restrict__ row_ptr, const int* __restrict__ col,
                                                       const float* __restrict__ val, const float* __restrict__ Y, int N, int S,
                                                       int np, const float* __restrict__ part, float* __restrict__ o_a,
                                                       float* __restrict__ o_b, float* __restrict__ o_z) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const float2 yi = reinterpret_cast<const float2*>(Y)[i];
  const int e1 = row_ptr[i + 1];
  float a0 = 0.f, a1 = 0.f;
  for (int e = row_ptr[i] + lane; e < e1; e += 64) {
    const float p = val[e];
    const float2 yj = reinterpret_cast<const float2*>(Y)[col[e]];
    const float dx = yi.x - yj.x, dy = yi.y - yj.y;
    const float q = dx * dx + dy * dy;
    if (MODE == 0) {
      const float pw = p * (1.f / (1.f + q));
      a0 = a0 + pw * dx;
      a1 = a1 + pw * dy;
    } else if (p > 0.f) {
      a0 = a0 + p * (logf(p) + logf(1.f + q));
      a1 = a1 + p;
    }
  }
  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  if (lane < 3) {  // lane c folds component c (rep x, rep y, Z_i) over the segments in ascending order
    float f = 0.f;
    for (int s = 0; s < S; ++s) f = f + part[((size_t)s * 3 + lane) * np + i];
    if (lane == 2) o_z[i] = f;
    else if (MODE == 0) o_b[2 * i + lane] = f;
  }
  if (lane == 0) {
    if (MODE == 0) o_a[2 * i] = a0, o_a[2 * i + 1] = a1;
    else o_a[i] = a0, o_b[i] = a1;
  }
}

inline bool nbr_n_ok(long N) { return N >= 4 && N <= NBR_MAX_N; }

}  // namespace

extern "C" int tacorl_tsne_nbr_max_n(void) { return NBR_MAX_N; }
extern "C" int tacorl_tsne_nbr_max_k(void) { return NBR_MAX_K; }
extern "C" int tacorl_tsne_nbr_knn_tile(void) { return NBR_KNN_TILE; }
extern "C" int tacorl_tsne_nbr_segment(long N) { return nbr_n_ok(N) ? nbr_segment((int)N) : 0; }
extern "C" int tacorl_tsne_nbr_supported(long N, int D, int K) {
  return nbr_n_ok(N) && D >= 1 && D <= TSNE_MAX_D && K >= 1 && K <= NBR_MAX_K && K <= N - 1;
}
extern "C" size_t tacorl_tsne_nbr_workspace_bytes(long N) { return nbr_n_ok(N) ? nbr_ws_layout((int)N).total : 0; }

extern "C" int tacorl_tsne_nbr_workspace_offsets(long N, long* off) {
  if (!nbr_n_ok(N) || !off) return TACORL_EINVAL;
  const NbrWsLayout w = nbr_ws_layout((int)N);
  off[0] = (long)w.xn, off[1] = (long)w.attr, off[2] = (long)w.rep, off[3] = (long)w.zrow;
  return TACORL_OK;
}

extern "C" int tacorl_tsne_nbr_knn(const float* points, long N, int D, long ld, int K, int* nbr_row, float* nbr_dist,
                                   tacorl_stream_t stream) {
  if (!tacorl_tsne_nbr_supported(N, D, K) || ld < D || bad_ptr(points, 3) || bad_ptr(nbr_row, 3) || bad_ptr(nbr_dist, 3))
    return TACORL_EINVAL;
  return nbr_knn_dispatch(points, (int)N, D, ld, K, nbr_row, nbr_dist, (hipStream_t)stream);
}

extern "C" int tacorl_tsne_nbr_affinities(const float* X, long N, int D, long ld, float perplexity, int* nbr_row, float* nbr_dist,
                                          float* cond, float* beta, int* row_ptr, int* col, float* val, long capacity, int* status,
                                          void* ws, size_t ws_bytes, tacorl_stream_t stream) {
  if (!nbr_n_ok(N) || !(perplexity >= 1.f) || !(perplexity <= (float)NBR_MAX_K)) return TACORL_EINVAL;
  const int K = (int)floorf(3.f * perplexity);
  if (!tacorl_tsne_nbr_supported(N, D, K) || ld < D || capacity < 2 * N * K) return TACORL_EINVAL;
  if (bad_ptr(X, 3) || bad_ptr(nbr_row, 3) || bad_ptr(nbr_dist, 3) || bad_ptr(cond, 3) || bad_ptr(beta, 3) || bad_ptr(row_ptr, 3) ||
      bad_ptr(col, 3) || bad_ptr(val, 3) || bad_ptr(status, 3) || bad_ptr(ws, 15) || ws_bytes < tacorl_tsne_nbr_workspace_bytes(N))
    return TACORL_EINVAL;
  const int n = (int)N;
  const hipStream_t st = (hipStream_t)stream;
  const NbrWsLayout w = nbr_ws_layout(n);
  float* xn = reinterpret_cast<float*>((char*)ws + w.xn);
  int* cnt = reinterpret_cast<int*>((char*)ws + w.cnt);
  hipLaunchKernelGGL(tsne_normalise_kernel, dim3(1), dim3(RED_T), 0, st, X, n, D, ld, xn, status);
  const int rc = nbr_knn_dispatch(xn, n, D, TSNE_XP, K, nbr_row, nbr_dist, st);
  if (rc != TACORL_OK) return rc;
  const dim3 rows((n + 3) / 4);
  hipLaunchKernelGGL(nbr_cond_kernel, rows, dim3(256), 0, st, nbr_dist, n, K, logf(perplexity), cond, beta, status);
  hipLaunchKernelGGL(nbr_zero_kernel, dim3((n + 255) / 256), dim3(256), 0, st, cnt, n);
  hipLaunchKernelGGL(nbr_count_kernel, rows, dim3(256), 0, st, nbr_row, n, K, cnt);
  hipLaunchKernelGGL(nbr_scan_kernel, dim3(1), dim3(RED_T), 0, st, n, K, cnt, row_ptr);
  hipLaunchKernelGGL(nbr_fill_kernel, rows, dim3(256), 0, st, nbr_row, cond, n, K, row_ptr, cnt, col, val);
  hipLaunchKernelGGL(nbr_sort_kernel, dim3(n), dim3(NBR_SORT_T), 0, st, row_ptr, col, val);
  return LAUNCH_OK();
}

namespace {
inline bool nbr_bad_common(const int* row_ptr, const int* col, const float* val, long N, const float* Y, void* ws, size_t ws_bytes) {
  return !nbr_n_ok(N) || bad_ptr(row_ptr, 3) || bad_ptr(col, 3) || bad_ptr(val, 3) || bad_ptr(Y, 7) || bad_ptr(ws, 15) ||
         ws_bytes < tacorl_tsne_nbr_workspace_bytes(N);
}
}  // namespace

extern "C" int tacorl_tsne_nbr_step(const int* row_ptr, const int* col, const float* val, long N, float* Y, float* u, float* gains,
                                    float exaggeration, float momentum, float lr, void* ws, size_t ws_bytes,
                                    tacorl_stream_t stream) {
  if (nbr_bad_common(row_ptr, col, val, N, Y, ws, ws_bytes) || bad_ptr(u, 3) || bad_ptr(gains, 3)) return TACORL_EINVAL;
  const int n = (int)N;
  const hipStream_t st = (hipStream_t)stream;
  const NbrWsLayout w = nbr_ws_layout(n);
  char* b = (char*)ws;
  float *attr = (float*)(b + w.attr), *rep = (float*)(b + w.rep), *zrow = (float*)(b + w.zrow), *scal = (float*)(b + w.scal);
  float* part = (float*)(b + w.part);
  const int seg = nbr_segment(n), S = (n + seg - 1) / seg, np = (n + 3) & ~3;
  hipLaunchKernelGGL(nbr_rep_kernel, dim3((n + NBR_REP_T - 1) / NBR_REP_T, S), dim3(NBR_REP_T), 0, st, Y, n, seg, np, part);
  hipLaunchKernelGGL(nbr_rows_kernel<0>, dim3((n + 3) / 4), dim3(256), 0, st, row_ptr, col, val, Y, n, S, np, part, attr, rep, zrow);
  hipLaunchKernelGGL(tsne_update_kernel, dim3(1), dim3(RED_T), 0, st, n, Y, u, gains, attr, rep, zrow, exaggeration, momentum, lr,
                     scal);
  return LAUNCH_OK();
}

extern "C" int tacorl_tsne_nbr_kl(const int* row_ptr, const int* col, const float* val, const float* Y, long N, float* out, void* ws,
                                  size_t ws_bytes, tacorl_stream_t stream) {
  if (nbr_bad_common(row_ptr, col, val, N, Y, ws, ws_bytes) || bad_ptr(out, 3)) return TACORL_EINVAL;
  const int n = (int)N;
  const hipStream_t st = (hipStream_t)stream;
  const NbrWsLayout w = nbr_ws_layout(n);
  char* b = (char*)ws;
  float *krow = (float*)(b + w.krow), *prow = (float*)(b + w.prow), *zrow = (float*)(b + w.zrow), *part = (float*)(b + w.part);
  const int seg = nbr_segment(n), S = (n + seg - 1) / seg, np = (n + 3) & ~3;
  hipLaunchKernelGGL(nbr_rep_kernel, dim3((n + NBR_REP_T - 1) / NBR_REP_T, S), dim3(NBR_REP_T), 0, st, Y, n, seg, np, part);
  hipLaunchKernelGGL(nbr_rows_kernel<1>, dim3((n + 3) / 4), dim3(256), 0, st, row_ptr, col, val, Y, n, S, np, part, krow, prow, zrow);
  hipLaunchKernelGGL(tsne_kl_finish_kernel, dim3(1), dim3(RED_T), 0, st, n, krow, prow, zrow, out);
  return LAUNCH_OK();
}
