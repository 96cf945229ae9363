// The neighbour table of the `similar_robot_obs` goal strategy (reference set_nn_steps_from_step,
// datamodule/dataset/play_dataset.py:183-234, goal_cond_replay_buffer_dataset.py:76-130): an exact brute-force L2 k-NN of every
// frame's robot_obs against all frames, then the temporal margin filter.  The N x N distance matrix never exists.
//
// Definition (include/tacorl_hip.h tacorl_knn_l2): d(q, p) in fp32, sequentially over j, acc = acc + (q_j - p_j) * (q_j - p_j),
// every operation rounded once (no contraction: -ffp-contract=off); the neighbours of a query are the min(k, N) rows with the
// smallest (d, row), ascending.  Consecutive frames of a trajectory are near-duplicates, so the expanded form
// |q|^2 + |p|^2 - 2 q.p (MFMA / BLAS) would cancel on exactly the pairs the lists are made of; this is the direct form.
//
// Shape: one thread per query, the query's D floats in registers (D padded to DP = a multiple of 4 with zeros: a zero term
// adds +0 to a non-negative acc, so the padding changes no bit).  Database tiles of KNN_TILE rows are staged in LDS and read as
// ds_read_b128 broadcasts (all lanes read the same point: no bank conflict); the next tile's global loads are in flight during
// the current tile's arithmetic.  Each thread's sorted (d, row) list lives in LDS, slot-major ([slot][thread]: consecutive
// lanes on consecutive banks), and a candidate enters it only when it beats the thread's threshold register - after the
// warm-up that is ~k ln(N / k) insertions per query, so the inner loop is the 3 D VALU operations plus one compare per point.
// A thread scans rows in ascending order and inserts on "strictly below the threshold", which yields the lower-row tie-break.
#include "../../include/tacorl_hip.h"
#include "common.h"

#include <stdint.h>

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? TACORL_OK : TACORL_ELAUNCH)

namespace {

constexpr int KNN_TILE = 128;        // database rows per LDS tile
constexpr int KNN_MAX_D = 32;
constexpr int KNN_MAX_K = 64;
constexpr int KNN_NOT_FULL = 0x7f800001;  // threshold while the list has free slots: above the bits of +inf, admits every distance

inline int knn_query_block(int k) { return k <= 32 ? 256 : 128; }  // lists: block * k * 8 bytes <= 64 KiB

// Distances are >= +0 (a sum of squares from +0), so their bit patterns order as integers: one integer compare serves both
// "strictly below the k-th distance" and, while the list is not full, "anything, +inf included".
template <int DP, int T>
__global__ __launch_bounds__(T) void knn_l2_kernel(const float* __restrict__ points, int n_points, int D, long ld, long q0,
                                                   long n_queries, int k, int* __restrict__ nbr_row,
                                                   float* __restrict__ nbr_dist) {
  extern __shared__ __attribute__((aligned(16))) unsigned char knn_smem[];
  float* tile = reinterpret_cast<float*>(knn_smem);                    // [KNN_TILE][DP]
  float* ld_d = tile + KNN_TILE * DP;                                  // [k][T]
  int* ld_r = reinterpret_cast<int*>(ld_d + (size_t)k * T);            // [k][T]
  const int tid = threadIdx.x;
  const long qi = (long)blockIdx.x * T + tid;                          // query number inside the slice
  const bool live = qi < n_queries;
  const long qrow = q0 + (live ? qi : n_queries - 1);                  // (idle threads of the last block mirror its last query)

  float q[DP];
#pragma unroll
  for (int j = 0; j < DP; ++j) q[j] = j < D ? points[qrow * ld + j] : 0.f;
  for (int s = 0; s < k; ++s) {
    ld_d[s * T + tid] = __int_as_float(0x7f800000);
    ld_r[s * T + tid] = -1;
  }
  int thr = KNN_NOT_FULL;

  // a tile is KNN_TILE * DP floats; thread t stages elements t, t + T, ... (row = e / DP, column = e % DP)
  constexpr int NPRE = KNN_TILE * DP / T;
  static_assert(KNN_TILE * DP % T == 0, "tile elements divide over the block");
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
    thr = ld_r[(k - 1) * T + tid] >= 0 ? __float_as_int(ld_d[(k - 1) * T + tid]) : KNN_NOT_FULL;
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
    return acc;
  };

  fetch(0);
  for (int base = 0; base < n_points; base += KNN_TILE) {
    __syncthreads();  // every thread is done with the previous tile
#pragma unroll
    for (int i = 0; i < NPRE; ++i) tile[tid + i * T] = pre[i];
    __syncthreads();
    if (base + KNN_TILE < n_points) fetch(base + KNN_TILE);
    const int valid = n_points - base < KNN_TILE ? n_points - base : KNN_TILE;
    int r = 0;
    for (; r + 4 <= valid; r += 4) {  // four independent accumulation chains
      const float d0 = dist(tile + (r + 0) * DP), d1 = dist(tile + (r + 1) * DP);
      const float d2 = dist(tile + (r + 2) * DP), d3 = dist(tile + (r + 3) * DP);
      if (__float_as_int(d0) < thr) insert(d0, base + r + 0);
      if (__float_as_int(d1) < thr) insert(d1, base + r + 1);
      if (__float_as_int(d2) < thr) insert(d2, base + r + 2);
      if (__float_as_int(d3) < thr) insert(d3, base + r + 3);
    }
    for (; r < valid; ++r) {  // the masked tail: rows past n_points never enter a list
      const float d = dist(tile + r * DP);
      if (__float_as_int(d) < thr) insert(d, base + r);
    }
  }
  if (!live) return;
  for (int s = 0; s < k; ++s) {
    nbr_row[qi * k + s] = ld_r[s * T + tid];
    if (nbr_dist) nbr_dist[qi * k + s] = ld_d[s * T + tid];
  }
}

// nn_steps[q] = the steps of q's neighbour rows that lie at least `margin` steps away from q's own step, in list order,
// packed left and padded with -1; count[q] = how many.  One thread per query.
__global__ void nn_margin_filter_kernel(const int* __restrict__ nbr_row, long n_queries, int k, long q0,
                                        const long* __restrict__ step_of_row, long n_points, long margin,
                                        long* __restrict__ nn_steps, int* __restrict__ count) {
  const long qi = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (qi >= n_queries) return;
  const long t = step_of_row[q0 + qi];
  int n = 0;
  for (int s = 0; s < k; ++s) {
    const int r = nbr_row[qi * k + s];
    if (r < 0 || r >= n_points) continue;  // absent entry
    const long st = step_of_row[r];
    const long diff = t > st ? t - st : st - t;
    if (diff < margin) continue;           // st + margin > t > st - margin
    nn_steps[qi * k + n++] = st;
  }
  count[qi] = n;
  for (; n < k; ++n) nn_steps[qi * k + n] = -1;
}

template <int DP, int T>
int knn_launch(const float* points, int n_points, int D, long ld, long q0, long n_queries, int k, int* nbr_row, float* nbr_dist,
               hipStream_t st) {
  const size_t lds = (size_t)KNN_TILE * DP * 4 + (size_t)T * k * 8;
  static int attr = hipFuncSetAttribute(reinterpret_cast<const void*>(knn_l2_kernel<DP, T>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize,
                                        KNN_TILE * DP * 4 + 64 * 1024) == hipSuccess ? 0 : -1;
  if (attr != 0) return TACORL_ELAUNCH;
  const long blocks = (n_queries + T - 1) / T;
  hipLaunchKernelGGL((knn_l2_kernel<DP, T>), dim3((unsigned)blocks), dim3(T), lds, st, points, n_points, D, ld, q0, n_queries,
                     k, nbr_row, nbr_dist);
  return LAUNCH_OK();
}

template <int T>
int knn_dispatch(const float* points, int n_points, int D, long ld, long q0, long n_queries, int k, int* nbr_row,
                 float* nbr_dist, hipStream_t st) {
  switch ((D + 3) / 4) {
#define KNN_CASE(Q) \
  case Q:           \
    return knn_launch<4 * Q, T>(points, n_points, D, ld, q0, n_queries, k, nbr_row, nbr_dist, st);
    KNN_CASE(1) KNN_CASE(2) KNN_CASE(3) KNN_CASE(4) KNN_CASE(5) KNN_CASE(6) KNN_CASE(7) KNN_CASE(8)
#undef KNN_CASE
  }
  return TACORL_EINVAL;
}

}  // namespace

extern "C" int tacorl_knn_l2_supported(int D, int k) { return D >= 1 && D <= KNN_MAX_D && k >= 1 && k <= KNN_MAX_K; }
extern "C" int tacorl_knn_l2_tile(void) { return KNN_TILE; }
extern "C" int tacorl_knn_l2_query_block(int k) { return k >= 1 && k <= KNN_MAX_K ? knn_query_block(k) : 0; }

extern "C" int tacorl_knn_l2(const float* points, long n_points, int D, long ld, long q0, long n_queries, int k, int* nbr_row,
                             float* nbr_dist, tacorl_stream_t stream) {
  if (!tacorl_knn_l2_supported(D, k) || n_points <= 0 || n_points > 2147483647L || ld < D || n_queries <= 0 || q0 < 0 ||
      q0 > n_points - n_queries)
    return TACORL_EINVAL;
  if (!points || ((uintptr_t)points & 3) || !nbr_row || ((uintptr_t)nbr_row & 3) || ((uintptr_t)nbr_dist & 3)) return TACORL_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  return knn_query_block(k) == 256 ? knn_dispatch<256>(points, (int)n_points, D, ld, q0, n_queries, k, nbr_row, nbr_dist, st)
                                   : knn_dispatch<128>(points, (int)n_points, D, ld, q0, n_queries, k, nbr_row, nbr_dist, st);
}

extern "C" int tacorl_nn_margin_filter(const int* nbr_row, long n_queries, int k, long q0, const long* step_of_row,
                                       long n_points, long margin, long* nn_steps, int* count, tacorl_stream_t stream) {
  if (k < 1 || k > KNN_MAX_K || n_points <= 0 || n_points > 2147483647L || n_queries <= 0 || q0 < 0 ||
      q0 > n_points - n_queries || margin < 0)
    return TACORL_EINVAL;
  if (!nbr_row || ((uintptr_t)nbr_row & 3) || !count || ((uintptr_t)count & 3) || !step_of_row || ((uintptr_t)step_of_row & 7) ||
      !nn_steps || ((uintptr_t)nn_steps & 7))
    return TACORL_EINVAL;
  hipLaunchKernelGGL(nn_margin_filter_kernel, dim3((unsigned)((n_queries + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     nbr_row, n_queries, k, q0, step_of_row, n_points, margin, nn_steps, count);
  return LAUNCH_OK();
}
