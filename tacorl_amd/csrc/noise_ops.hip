// The noise of a training step from a counter-based generator: every element is a pure function of
// (seed, step, draw id, GLOBAL sample index, position inside the sample), so a step's noise does not depend on how
// many ranks share the batch, and (seed, step) is all a checkpoint has to keep (tacorl_amd/noise.py states the same
// function in NumPy; DESIGN.md "Device noise").  One launch fills every noise buffer of a step.
//
// Philox4x32-10 (Salmon et al., SC'11): key (seed lo, seed hi), counter (q, sample0 + b, draw_id << 16 | k, step) with
// q = j >> 2 the group of four inside the sample's `inner` elements; element j takes word j & 3.
#include <limits.h>

#include "../../include/tacorl_hip.h"
#include "common.h"

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? TACORL_OK : TACORL_ELAUNCH)

namespace {

constexpr int NOISE_WG = 256;  // threads (= groups of four) per workgroup

struct NoiseTbl {
  int n_seg, n_groups;
  tacorl_noise_seg s[TACORL_NOISE_MAX_SEGS];
};

__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

__device__ __forceinline__ float word_uniform(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }  // [0, 1), exact

// Box-Muller on a word pair: u1 = ((a >> 8) + 1) 2^-24 in (0, 1], angle 2 pi u2 with u2 = (b >> 8) 2^-24.  sincospif
// takes the exact argument 2 u2 (a 24-bit integer times 2^-23), so no fp32 range reduction of 2 pi u2 is involved.
__device__ __forceinline__ void word_pair_normal(uint32_t a, uint32_t b, float& z0, float& z1) {
  const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;
  const float r = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincospif((float)(b >> 8) * 0x1p-23f, &s, &c);
  z0 = r * c;
  z1 = r * s;
}

// One thread per group of four elements; groups of all segments are numbered densely (s.group0 = groups in front of
// the segment), so every workgroup but the last has 256 groups of work whatever the segments' sizes.
__global__ __launch_bounds__(NOISE_WG) void noise_fill_kernel(NoiseTbl t, float* __restrict__ base_f32,
                                                              unsigned char* __restrict__ base_u8, uint32_t key0,
                                                              uint32_t key1, uint32_t step, uint32_t sample0) {
  const int g = blockIdx.x * NOISE_WG + threadIdx.x;
  if (g >= t.n_groups) return;
  int lo = 0, hi = t.n_seg - 1;  // last segment whose group0 <= g
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t.s[mid].group0 <= g) lo = mid; else hi = mid - 1;
  }
  const tacorl_noise_seg sg = t.s[lo];
  const int qn = (sg.inner + 3) >> 2;
  const int gl = g - sg.group0;
  const int q = gl % qn, row = gl / qn;  // row: (b, k) in the segment's own order
  int b, k;
  if (sg.outer_major) { k = row / sg.B_local; b = row - k * sg.B_local; }
  else { b = row / sg.n_outer; k = row - b * sg.n_outer; }
  uint32_t w[4] = {(uint32_t)q, sample0 + (uint32_t)b, ((uint32_t)sg.draw_id << 16) | (uint32_t)k, step};
  philox4x32_10(w, key0, key1);
  const int j0 = q << 2;
  const int nj = min(4, sg.inner - j0);
  const long at = (long)sg.offset + (long)row * sg.inner + j0;
  if (sg.kind == TACORL_NOISE_KEEP) {
    unsigned char* d = base_u8 + at;
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (i < nj) d[i] = word_uniform(w[i]) < sg.keep_p ? 1 : 0;
    return;
  }
  float v[4];
  if (sg.kind == TACORL_NOISE_NORMAL) {
    word_pair_normal(w[0], w[1], v[0], v[1]);
    word_pair_normal(w[2], w[3], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = word_uniform(w[i]);
  }
  float* d = base_f32 + at;
  if (nj == 4 && (at & 3) == 0) {  // (base_f32 is 16-byte aligned: checked by the entry point)
    *reinterpret_cast<f32x4*>(d) = f32x4{v[0], v[1], v[2], v[3]};
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (i < nj) d[i] = v[i];
}

// ---- a rollout step's draws: sample and step word per row (tacorl_hip.h, tacorl_noise_fill_rows) ----
// The table travels by value; rowlist[s] lists the rows of segment s's mask in ascending order, so the groups of a launch
// are numbered densely over the rows that are drawn and a row outside the mask costs no thread.
struct RowsTbl {
  int n_seg, n_groups;
  int group0[TACORL_NOISE_ROWS_SEGS], offset[TACORL_NOISE_ROWS_SEGS], kind[TACORL_NOISE_ROWS_SEGS];
  int inner[TACORL_NOISE_ROWS_SEGS], which[TACORL_NOISE_ROWS_SEGS];
  uint32_t ctr2[TACORL_NOISE_ROWS_SEGS];  // draw_id << 16
  uint32_t episode[TACORL_NOISE_ROWS_MAX];
  uint32_t number[2][TACORL_NOISE_ROWS_MAX];  // [0]: step, [1]: plan_no
  unsigned char rowlist[TACORL_NOISE_ROWS_SEGS][TACORL_NOISE_ROWS_MAX];
};

__global__ __launch_bounds__(NOISE_WG) void noise_fill_rows_kernel(RowsTbl t, float* __restrict__ base_f32, uint32_t key0,
                                                                   uint32_t key1) {
  const int g = blockIdx.x * NOISE_WG + threadIdx.x;
  if (g >= t.n_groups) return;
  int s = 0;  // last segment whose group0 <= g (an empty segment shares its group0 with the next one: the last one wins)
#pragma unroll
  for (int i = 1; i < TACORL_NOISE_ROWS_SEGS; i++)
    if (i < t.n_seg && t.group0[i] <= g) s = i;
  const int inner = t.inner[s];
  const int qn = (inner + 3) >> 2;
  const int gl = g - t.group0[s];
  const int q = gl % qn;
  const int row = t.rowlist[s][gl / qn];
  uint32_t w[4] = {(uint32_t)q, t.episode[row], t.ctr2[s], t.number[t.which[s]][row]};
  philox4x32_10(w, key0, key1);
  float v[4];
  if (t.kind[s] == TACORL_NOISE_NORMAL) {
    word_pair_normal(w[0], w[1], v[0], v[1]);
    word_pair_normal(w[2], w[3], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = word_uniform(w[i]);
  }
  const int j0 = q << 2;
  const int nj = min(4, inner - j0);
  const long at = (long)t.offset[s] + (long)row * inner + j0;  // < n_f32: checked by the entry point
  float* d = base_f32 + at;
  if (nj == 4 && (at & 3) == 0) {  // (base_f32 is 16-byte aligned: checked by the entry point)
    *reinterpret_cast<f32x4*>(d) = f32x4{v[0], v[1], v[2], v[3]};
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (i < nj) d[i] = v[i];
}

}  // namespace

extern "C" int tacorl_noise_fill_rows(const void* rows, void* base_f32, unsigned long long seed, tacorl_stream_t stream) {
  if (rows == nullptr || base_f32 == nullptr || ((uintptr_t)base_f32 & 15) != 0) return TACORL_EINVAL;
  const tacorl_noise_rows* in = static_cast<const tacorl_noise_rows*>(rows);
  const int R = in->n_rows;
  if (R < 1 || R > TACORL_NOISE_ROWS_MAX || in->n_seg < 1 || in->n_seg > TACORL_NOISE_ROWS_SEGS) return TACORL_EINVAL;
  if (in->n_f32 < 0 || in->reserved != 0) return TACORL_EINVAL;
  RowsTbl t{};
  t.n_seg = in->n_seg;
  long groups = 0;
  for (int i = 0; i < in->n_seg; i++) {
    const tacorl_noise_rows_seg& s = in->seg[i];
    if (s.kind != TACORL_NOISE_NORMAL && s.kind != TACORL_NOISE_UNIFORM) return TACORL_EINVAL;
    if (s.which != 0 && s.which != 1) return TACORL_EINVAL;
    if (s.draw_id < 0 || s.draw_id > 65535 || s.inner < 1 || s.offset < 0 || s.reserved != 0) return TACORL_EINVAL;
    if ((long)s.offset + (long)R * s.inner > (long)in->n_f32) return TACORL_EINVAL;  // (so inner <= INT_MAX - 3 too)
    if (R < 64 && (s.mask >> R) != 0) return TACORL_EINVAL;
    t.group0[i] = (int)groups;
    t.offset[i] = s.offset;
    t.kind[i] = s.kind;
    t.inner[i] = s.inner;
    t.which[i] = s.which;
    t.ctr2[i] = (uint32_t)s.draw_id << 16;
    int n = 0;
    for (int r = 0; r < R; r++)
      if ((s.mask >> r) & 1ull) t.rowlist[i][n++] = (unsigned char)r;
    groups += (long)n * (((long)s.inner + 3) / 4);
    if (groups > (long)INT_MAX - NOISE_WG) return TACORL_EINVAL;
  }
  if (groups == 0) return TACORL_OK;  // every mask empty: nothing to draw
  t.n_groups = (int)groups;
  for (int r = 0; r < R; r++) {
    t.episode[r] = in->episode[r];
    t.number[0][r] = in->step[r];
    t.number[1][r] = in->plan_no[r];
  }
  hipLaunchKernelGGL(noise_fill_rows_kernel, dim3(cdiv(groups, NOISE_WG)), dim3(NOISE_WG), 0, (hipStream_t)stream, t,
                     (float*)base_f32, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
  return LAUNCH_OK();
}

extern "C" int tacorl_noise_fill(const void* segs, int n_seg, void* base_f32, void* base_u8, unsigned long long seed,
                                 unsigned int step, int sample0, tacorl_stream_t stream) {
  if (segs == nullptr || n_seg < 1 || n_seg > TACORL_NOISE_MAX_SEGS || sample0 < 0) return TACORL_EINVAL;
  const tacorl_noise_table* tab = static_cast<const tacorl_noise_table*>(segs);
  if (tab->n_f32 < 0 || tab->n_u8 < 0 || tab->reserved != 0) return TACORL_EINVAL;
  if (((uintptr_t)base_f32 & 15) != 0) return TACORL_EINVAL;
  NoiseTbl t{};
  t.n_seg = n_seg;
  long groups = 0;
  for (int i = 0; i < n_seg; i++) {
    const tacorl_noise_seg& s = tab->seg[i];
    if (s.kind != TACORL_NOISE_NORMAL && s.kind != TACORL_NOISE_UNIFORM && s.kind != TACORL_NOISE_KEEP) return TACORL_EINVAL;
    if (s.draw_id < 0 || s.draw_id > 65535 || s.n_outer < 1 || s.n_outer > 65535 || s.B_local < 1 || s.inner < 1) return TACORL_EINVAL;
    if (s.outer_major != 0 && s.outer_major != 1) return TACORL_EINVAL;
    if (s.offset < 0 || s.reserved != 0) return TACORL_EINVAL;
    if ((long)sample0 + s.B_local > (long)INT_MAX) return TACORL_EINVAL;
    const long rows = (long)s.n_outer * s.B_local;  // < 2^47
    if (s.inner > INT_MAX / 4 || rows > (long)INT_MAX) return TACORL_EINVAL;
    const long elems = rows * s.inner;  // < 2^62
    const bool u8 = s.kind == TACORL_NOISE_KEEP;
    if (u8 ? base_u8 == nullptr : base_f32 == nullptr) return TACORL_EINVAL;
    if (u8 && !(s.keep_p >= 0.0f && s.keep_p <= 1.0f)) return TACORL_EINVAL;
    if (s.offset + elems > (long)(u8 ? tab->n_u8 : tab->n_f32)) return TACORL_EINVAL;
    if (s.group0 != groups) return TACORL_EINVAL;
    groups += rows * ((s.inner + 3) / 4);
    if (groups > (long)INT_MAX - NOISE_WG) return TACORL_EINVAL;
    t.s[i] = s;
  }
  if (groups != tab->n_groups) return TACORL_EINVAL;
  t.n_groups = (int)groups;
  hipLaunchKernelGGL(noise_fill_kernel, dim3(cdiv(groups, NOISE_WG)), dim3(NOISE_WG), 0, (hipStream_t)stream, t, (float*)base_f32,
                     (unsigned char*)base_u8, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), (uint32_t)step,
                     (uint32_t)sample0);
  return LAUNCH_OK();
}
