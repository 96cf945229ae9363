// Replay data path on the GPU: the dataset's uint8 HWC frames stay resident in HBM
// (a CALVIN-sized play dataset is ~50 GB of 84x84x3 frames: it fits in one MI355X's 288 GB), a step's windows are
// gathered by frame index, and the reference's train-time image pipeline runs on the way into the encoder's NHWC
// image buffers: RandomShiftsAug -> x/255 -> ColorJitter(brightness, contrast, hue) -> Normalize(0.5, 0.5)
// (config/datamodule/transform_manager/transforms/rl_train.yaml; utils/transforms.py:265-330).  All random draws are
// explicit inputs (per-image tables), so the kernels are deterministic functions that goldens can pin.
// Pure byte / elementwise work: HBM-bound, coalesced 16-byte accesses, no MFMA.
#include "../../include/tacorl_hip.h"
#include "bilinear.h"
#include "common.h"

#include <initializer_list>

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? TACORL_OK : TACORL_ELAUNCH)

namespace {

// dst[i] = frames[index[i]] : n frames of frame_bytes (multiple of 16), one 16-byte chunk per thread iteration
__global__ void gather_frames_u8_kernel(const unsigned char* __restrict__ base, long frame_bytes, const long* __restrict__ index,
                                        unsigned char* __restrict__ dst, long n, int chunks) {
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const long total = n * chunks;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const long i = q / chunks;
    const int c = (int)(q - i * chunks);
    *reinterpret_cast<u32x4*>(dst + i * frame_bytes + (long)c * 16) =
        *reinterpret_cast<const u32x4*>(base + index[i] * frame_bytes + (long)c * 16);
  }
}

// torchvision.transforms.functional (_functional_tensor.py) colour operations on one RGB pixel in [0, 1]
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
__device__ __forceinline__ float gray_of(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }
__device__ __forceinline__ void adjust_hue(float& r, float& g, float& b, float hf) {
  // _rgb2hsv
  const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
  const bool eqc = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eqc ? 1.f : maxc);
  const float div = eqc ? 1.f : cr;
  const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
  const float hr = (maxc == r) ? (bc - gc) : 0.f;
  const float hg = ((maxc == g) && (maxc != r)) ? (2.f + rc - bc) : 0.f;
  const float hb = ((maxc != g) && (maxc != r)) ? (4.f + gc - rc) : 0.f;
  float h = fmodf((hr + hg + hb) / 6.f + 1.f, 1.f);
  // shift: (h + hue_factor) % 1.0 with python's non-negative remainder
  h = h + hf;
  h = h - floorf(h);
  // _hsv2rgb
  const float v = maxc;
  const float h6 = h * 6.f, fi = floorf(h6), f = h6 - fi;
  const int i = ((int)fi) % 6;
  const float p = clamp01(v * (1.f - s)), q = clamp01(v * (1.f - f * s)), t = clamp01(v * (1.f - (1.f - f) * s));
  switch (i) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

struct AugJob {
  const unsigned char* src;  // uint8 HWC frames
  long pitch;                // bytes between frames
  void* dst;                 // NHWC normalised frames
  const int* shift;          // [n][2] (sx, sy) in [0, 2*pad], or NULL: no shift
  const float* jitter;       // [n][8] {brightness, contrast, hue, order0..3, apply}, or NULL: no colour jitter
  const long* idx;           // optional frame ids: image i is frame idx[i * istride] of the dataset at src
  int istride;
  int n;
};
#define AUG_MAXJ 8
struct AugTbl { AugJob j[AUG_MAXJ]; };

// One workgroup per image.  RandomShiftsAug with integer shifts = a clamped (replicate-padded) translation; the
// colour operations run in the drawn order; adjust_contrast needs the image's mean grey level AFTER the operations
// that precede it, hence the first pass (a block reduction) when contrast is drawn.
// The Resize stage (rl_train.yaml:3-4,16-17: 200x200 -> 128x128 static, -> 84x84 gripper, applied to the 0..255 float frame
// BEFORE RandomShiftsAug) samples by the rule of bilinear.h, which the store-time resize (frame_ops.hip) shares.
template <typename OutT>
__global__ __launch_bounds__(256) void pack_u8_aug_kernel(AugTbl t, int H, int W, int pad, int Hs, int Ws) {
  const AugJob jb = t.j[blockIdx.y];
  const int img = blockIdx.x;
  if (img >= jb.n) return;
  __shared__ float red[4];
  const unsigned char* __restrict__ src = jb.src + (jb.idx ? jb.idx[(long)img * jb.istride] : (long)img) * jb.pitch;
  OutT* __restrict__ dst = reinterpret_cast<OutT*>(jb.dst) + (long)img * H * W * 3;
  const int sx = jb.shift ? jb.shift[2 * img] - pad : 0, sy = jb.shift ? jb.shift[2 * img + 1] - pad : 0;
  float bf = 1.f, cf = 1.f, hf = 0.f;
  unsigned ord = 0u;  // the drawn order, 2 bits per position: op k = (ord >> 2k) & 3
  int cpos = 4;       // position of the contrast operation
  bool jit = false;
  if (jb.jitter) {
    const float* p = jb.jitter + 8L * img;
    bf = p[0]; cf = p[1]; hf = p[2];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const unsigned op = (unsigned)(int)p[3 + k] & 3u;
      ord |= op << (2 * k);
      if (op == 1u) cpos = k;
    }
    jit = p[7] != 0.f;
  }
  const int npx = H * W;
  const bool resize = Hs != H || Ws != W;
  const float sch = (float)Hs / (float)H, scw = (float)Ws / (float)W;
  auto load = [&](int px, float& r, float& g, float& b) {
    const int y = px / W, x = px - y * W;
    const int ys = min(max(y + sy, 0), H - 1), xs = min(max(x + sx, 0), W - 1);  // RandomShiftsAug on the (resized) frame
    if (!resize) {
      const unsigned char* s = src + ((long)ys * W + xs) * 3;
      r = (float)s[0] / 255.0f; g = (float)s[1] / 255.0f; b = (float)s[2] / 255.0f;  // ScaleImageTensor / ToTensor
      return;
    }
    int y0, y1, x0, x1;
    float h0, h1, w0, w1;
    bilinear_axis(ys, sch, Hs, y0, y1, h0, h1);
    bilinear_axis(xs, scw, Ws, x0, x1, w0, w1);
    const unsigned char *p00 = src + ((long)y0 * Ws + x0) * 3, *p01 = src + ((long)y0 * Ws + x1) * 3,
                        *p10 = src + ((long)y1 * Ws + x0) * 3, *p11 = src + ((long)y1 * Ws + x1) * 3;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; c++)
      v[c] = bilinear_mix(h0, h1, w0, w1, p00[c], p01[c], p10[c], p11[c]);
    r = v[0] / 255.0f; g = v[1] / 255.0f; b = v[2] / 255.0f;
  };
  float mean = 0.f;
  if (jit) {
    float part = 0.f;
    for (int px = threadIdx.x; px < npx; px += 256) {
      float r, g, b;
      load(px, r, g, b);
      for (int k = 0; k < cpos; k++) {  // the operations drawn before the contrast adjustment
        const unsigned op = (ord >> (2 * k)) & 3u;
        if (op == 0u) { r = clamp01(bf * r); g = clamp01(bf * g); b = clamp01(bf * b); }
        else if (op == 3u) adjust_hue(r, g, b, hf);
      }
      part += gray_of(r, g, b);
    }
    part = wave_sum(part);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    mean = (((red[0] + red[1]) + red[2]) + red[3]) / (float)npx;
  }
  for (int px = threadIdx.x; px < npx; px += 256) {
    float r, g, b;
    load(px, r, g, b);
    if (jit) {
      for (int k = 0; k < 4; k++) {
        const unsigned op = (ord >> (2 * k)) & 3u;
        if (op == 0u) { r = clamp01(bf * r); g = clamp01(bf * g); b = clamp01(bf * b); }
        else if (op == 1u) { r = clamp01(cf * r + (1.f - cf) * mean); g = clamp01(cf * g + (1.f - cf) * mean); b = clamp01(cf * b + (1.f - cf) * mean); }
        else if (op == 3u) adjust_hue(r, g, b, hf);
      }
    }
    r = (r - 0.5f) / 0.5f; g = (g - 0.5f) / 0.5f; b = (b - 0.5f) / 0.5f;  // Normalize(0.5, 0.5)
    dst[3L * px] = (OutT)r; dst[3L * px + 1] = (OutT)g; dst[3L * px + 2] = (OutT)b;
  }
}

// Transition sampling (reference datamodule/dataset/goal_cond_replay_buffer_dataset.py:145-299) as index arithmetic: one
// thread per sample.  The tables were validated on the host (tacorl_amd/data/replay.py TransitionIndex), so every id below
// lies in [0, n_frames) by construction; the clamps are a second line of defence in front of the unchecked frame gathers,
// and a clamp that had to change a value raises the status word (plain store: every writer stores the same 1).
struct TransTbl {
  const long* steps; long n_steps;              // possible_steps, sorted
  const long* ep_start; const long* ep_end; int n_ep;
  const long* nn_ptr; long n_nn; const long* nn_val;  // CSR neighbour lists of steps [0, n_nn)
  const float* actions;                         // (n_frames, A)
  const long* idx; const long* strategy; const long* disp; const double* u;
  long horizon, n_frames;
  long* ids; float* action; float* reward; float* done; int* status;
};
enum { TS_GEOMETRIC = 0, TS_SIMILAR = 1, TS_RANDOM = 2, TS_HORIZON = 3, TS_EPISODE = 4, TS_NEXT = 5 };

__device__ __forceinline__ long pick_of(double u, long n) {  // floor(u * n) kept inside [0, n)
  long k = (long)(u * (double)n);
  return k < 0 ? 0 : (k > n - 1 ? n - 1 : k);
}

// What the four samplers below share.
// v kept inside [lo, hi]; a clamp that had to change it sets `bad` (the status word).
__device__ __forceinline__ long clamped(long v, long lo, long hi, bool& bad) {
  if (v < lo || v > hi) { bad = true; v = v < lo ? lo : hi; }
  return v;
}

// The index of the last episode whose start is <= step (binary search over the sorted starts), -1 where there is none.
__device__ __forceinline__ int episode_of(const long* ep_start, int n_ep, long step) {
  int lo = 0, hi = n_ep;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ep_start[mid] <= step) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

// How the two wavefront-per-window kernels begin: item b's position in the lookup table, its window size in
// [min_window, Tmax] and its first frame s, so that the rows s .. s + ws - 1 exist.
struct Window { long pos; int ws; long s; };
__device__ __forceinline__ Window window_of(const long* idx, const long* window, const long* lookup, long n_items, long n_frames,
                                            int b, int min_window, int Tmax, bool& bad) {
  Window w;
  w.pos = clamped(idx[b], 0, n_items - 1, bad);
  w.ws = (int)clamped(window[b], min_window, Tmax, bad);
  w.s = clamped(lookup[w.pos], 0, n_frames - w.ws, bad);
  return w;
}

// Every pointer non-null (unless it may be absent) and aligned to `align` bytes, a power of two.
bool pointers_ok(std::initializer_list<const void*> ps, uintptr_t align, bool may_be_null = false) {
  for (const void* p : ps)
    if ((!p && !may_be_null) || ((uintptr_t)p & (align - 1))) return false;
  return true;
}

__global__ __launch_bounds__(256) void sample_transitions_kernel(TransTbl t, int B, int A) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  bool bad = false;
  const long pos = clamped(t.idx[b], 0, t.n_steps - 1, bad);
  const long step = t.steps[pos];
  const int ep = episode_of(t.ep_start, t.n_ep, step);
  const long end = t.ep_end[ep > 0 ? ep : 0];
  const double u = t.u[b];
  long strat = t.strategy[b];
  long goal = step + 1;
  bool fallback = false;  // the reference's `return self.get_goal_step(step, strategy="random")`
  if (strat == TS_GEOMETRIC) {
    const long d = t.disp[b];
    goal = d >= end - step ? end : step + d;  // min(end, step + disp) without the overflow of a huge draw
  } else if (strat == TS_SIMILAR) {
    long cnt = 0, first = 0;
    if (step >= 0 && step < t.n_nn) { first = t.nn_ptr[step]; cnt = t.nn_ptr[step + 1] - first; }
    if (cnt > 0) goal = t.nn_val[first + pick_of(u, cnt)];
    else fallback = true;
  } else if (strat == TS_HORIZON || strat == TS_EPISODE) {
    const long last = (strat == TS_HORIZON && t.horizon < end - step) ? step + t.horizon : end;
    if (last > step) goal = step + 1 + pick_of(u, last - step);
    else fallback = true;
  } else if (strat == TS_RANDOM) {
    fallback = true;
  } else if (strat != TS_NEXT) {
    bad = true;
  }
  if (fallback) {
    if (t.n_steps > 1) {
      const long j = pick_of(u, t.n_steps - 1);
      goal = t.steps[j + (j >= pos ? 1 : 0)];  // possible_steps with `step` removed, as an index shift
    } else {
      bad = true;
    }
  }
  const long top = t.n_frames - 1;
  long id[3] = {step, step + 1, goal};
#pragma unroll
  for (int k = 0; k < 3; k++) t.ids[(long)k * B + b] = id[k] = clamped(id[k], 0, top, bad);
  const float r = goal == step + 1 ? 1.f : 0.f;
  t.reward[b] = r;
  t.done[b] = r;
  const float* __restrict__ a = t.actions + id[0] * A;
  for (int k = 0; k < A; k++) t.action[(long)b * A + k] = a[k];
  if (bad) *t.status = 1;
}

// Relay sampling (reference datamodule/dataset/relay_imitation_learning_dataset.py:73-113) as index arithmetic: one thread per
// sample, in the form of sample_transitions_kernel.  Validated on the host (tacorl_amd/data/relay_replay.py RelayIndex); the
// clamps stand in front of every table access all the same - idx before the lookup read, every id before the action read and
// the frame gathers behind this kernel - and a clamp that changed a value raises the status word (plain store).
struct RelayTbl {
  const long* lookup; long n_items;             // episode_lookup: item -> step
  const long* ep_start; const long* ep_end; int n_ep;
  const float* actions; long n_frames;          // (n_frames, A)
  const long* idx; const double* u_low; const double* u_high;
  long low_window, high_window;
  long* ids; float* action; int* status;
};

__global__ __launch_bounds__(256) void sample_relay_kernel(RelayTbl t, int B, int A) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  bool bad = false;
  const long pos = clamped(t.idx[b], 0, t.n_items - 1, bad);
  const long top = t.n_frames - 1;
  const long step = clamped(t.lookup[pos], 0, top, bad);
  const int ep = episode_of(t.ep_start, t.n_ep, step);
  const long end = clamped(t.ep_end[ep > 0 ? ep : 0], step, top, bad);
  // min(end, step + window) without the overflow of a huge window
  const long sub = t.low_window >= end - step ? end : step + t.low_window;    // the subgoal frame (high_level_action)
  const long hmax = t.high_window >= end - step ? end : step + t.high_window;
  // sample_goal_step(start, stop): uniform over [start, stop) where that is not empty, else stop
  const long nl = sub - step - 1, nh = hmax - sub;
  const long low = nl > 0 ? step + 1 + pick_of(t.u_low[b], nl) : sub;
  const long high = nh > 0 ? sub + pick_of(t.u_high[b], nh) : hmax;
  const long id[4] = {step, low, high, sub};  // obs | low_level_goal | high_level_goal | high_level_action
#pragma unroll
  for (int k = 0; k < 4; k++) t.ids[(long)k * B + b] = clamped(id[k], 0, top, bad);
  const float* __restrict__ a = t.actions + step * A;
  for (int k = 0; k < A; k++) t.action[(long)b * A + k] = a[k];
  if (bad) *t.status = 1;
}

// Window sampling of the vector-observation dataset (reference datamodule/dataset/d4rl_play_dataset.py:69-146) over resident
// tables: one 64-lane wavefront per window, four windows per block.  The index arithmetic is uniform over the wavefront (the
// window id is made a scalar, so the table reads are scalar loads); the lanes then copy the window's rows - one contiguous span
// of ws * S floats in the table and in the batch - as coalesced dwords (S = 29: a span is 4-byte aligned only) and write the
// padding rows.  Validated on the host (tacorl_amd/data/d4rl_replay.py D4RLWindowIndex); the clamps stand in front of every
// table access all the same, and a clamp that changed a value raises the status word (plain store: every writer stores 1).
struct D4rlTbl {
  const long* lookup; long n_items;             // episode_lookup: item -> first frame of its window
  const long* ep_start; const long* ep_end; int n_ep;
  const float* observations; const float* actions; long n_frames;  // (n_frames, S), (n_frames, A)
  const long* idx; const long* window; const long* disp;
  float* obs; float* act; float* goal; float* reached; float* done; long* window_size; long* ids; int* status;
};

__global__ __launch_bounds__(256) void sample_d4rl_windows_kernel(D4rlTbl t, int B, int Tmax, int S, int A, int G, int min_window,
                                                                  float threshold) {
  const int b = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  bool bad = false;
  const Window w = window_of(t.idx, t.window, t.lookup, t.n_items, t.n_frames, b, min_window, Tmax, bad);
  const int ws = w.ws;
  const long s = w.s;
  long goal_step = s;
  if (G > 0) {
    const int ep = episode_of(t.ep_start, t.n_ep, s);
    const long end = t.ep_end[ep > 0 ? ep : 0];
    long d = t.disp[b];
    if (d < 1) { bad = true; d = 1; }
    // min(end, s + (ws - 1) * disp) without the overflow of a huge draw: the product is formed only where it stays <= end
    const long stride = ws - 1;
    goal_step = (stride == 0 || end < s || d > (end - s) / stride) ? (stride == 0 ? s : end) : s + stride * d;
    goal_step = clamped(goal_step, 0, t.n_frames - 1, bad);
  }
  {
    const float* __restrict__ src = t.observations + s * S;
    float* __restrict__ dst = t.obs + (long)b * Tmax * S;
    const int n = ws * S, last = n - S, pad = (Tmax - ws) * S;
    for (int i = lane; i < n; i += 64) dst[i] = src[i];
    for (int i = lane; i < pad; i += 64) dst[n + i] = src[last + i % S];  // pad_with_repetition: the window's last row
  }
  {
    const float* __restrict__ src = t.actions + s * A;
    float* __restrict__ dst = t.act + (long)b * Tmax * A;
    const int n = ws * A, pad = (Tmax - ws) * A;
    for (int i = lane; i < n; i += 64) dst[i] = src[i];
    for (int i = lane; i < pad; i += 64) dst[n + i] = 0.f;  // pad_with_zeros
  }
  if (lane != 0) return;
  if (G > 0) {
    const float* __restrict__ g = t.observations + goal_step * S;
    const float* __restrict__ e = t.observations + (s + ws - 1) * S;
    if (t.goal)
      for (int k = 0; k < G; k++) t.goal[(long)b * G + k] = g[k];
    // ||goal - observations[s + ws - 1][:2]|| < goal_threshold in fp32, the products and the sum rounded one by one
    const float dx = g[0] - e[0], dy = g[1] - e[1];
    const float r = sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy))) < threshold ? 1.f : 0.f;
    if (t.reached) t.reached[b] = r;
    if (t.done) t.done[b] = r;
  }
  if (t.window_size) t.window_size[b] = ws;
  if (t.ids) { t.ids[b] = s; t.ids[(long)B + b] = goal_step; }
  if (bad) *t.status = 1;
}

// Play-window sampling (reference datamodule/dataset/play_dataset.py:115-169,258-310; tacorl_amd/data/replay.py
// PlayIndex.sample + pad_actions) over resident tables, in the form of sample_d4rl_windows_kernel: one 64-lane wavefront per
// window, four windows per block, the index arithmetic uniform over the wavefront (scalar table reads).  The lanes then write
// the window's Tmax frame ids and copy its action rows - one contiguous span of ws * A floats in the table and in the batch -
// as coalesced dwords, and write the padding rows (zero, the gripper column repeated).  Validated on the host
// (tacorl_amd/data/play_replay.py validate_play_tables); the clamps stand in front of every table access all the same, and a
// clamp that changed a value raises the status word (plain store: every writer stores 1).
struct PlayTbl {
  const long* lookup; long n_items;             // episode_lookup: item -> first frame of its window
  const long* ep_start; const long* ep_end; int n_ep;
  const long* nn_ptr; long n_nn; const long* nn_val;  // CSR neighbour lists of frames [0, n_nn)
  const float* actions; long n_frames, last_end;      // (n_frames, A); the goal's clip bound max(ep_end)
  const long* idx; const long* window; const long* strategy; const long* disp; const long* noise;
  const double* u_choice; const double* u_random;
  long* ids; float* act; long* disp_out; long* window_size; int* status;
};

__global__ __launch_bounds__(256) void sample_play_windows_kernel(PlayTbl t, int B, int Tmax, int A, int min_window) {
  const int b = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  bool bad = false;
  const long top = t.n_frames - 1;
  const Window w = window_of(t.idx, t.window, t.lookup, t.n_items, t.n_frames, b, min_window, Tmax, bad);
  const int ws = w.ws;
  const long s = w.s;
  const long strat = clamped(t.strategy[b], 0, 1, bad);
  long d = t.disp[b];
  if (d < 1) { bad = true; d = 1; }
  // the random state (play_dataset.py:262-264): another item's first frame
  const long rs = clamped(t.lookup[pick_of(t.u_random[b], t.n_items)], 0, top, bad);
  long goal;
  if (strat == 0) {
    // find_episode_end: -1 where s lies in no episode (before the first start, or behind the end of the one found)
    const int ep = episode_of(t.ep_start, t.n_ep, s);
    const long end = ep >= 0 ? t.ep_end[ep] : -1;
    if (end < s) {
      goal = rs;
    } else {
      const long nz = clamped(t.noise ? t.noise[b] : 0, -1, 1, bad);
      // min(end, s + (ws - 1) * disp + noise) without the overflow of a huge draw: the product is formed only where the sum
      // stays <= end, i.e. (ws - 1) * disp <= lim; a one-frame window has stride 0 and is not divided by
      const long stride = ws - 1, lim = end - s - nz;
      if (lim < 0) goal = end;
      else if (stride == 0) goal = s + nz;
      else goal = d > lim / stride ? end : s + stride * d + nz;
    }
  } else {
    const long key = s + ws - 1;
    long first = 0, cnt = 0, total = 0;
    if (t.n_nn > 0) total = t.nn_ptr[t.n_nn];
    if (key >= 0 && key < t.n_nn) { first = t.nn_ptr[key]; cnt = t.nn_ptr[key + 1] - first; }
    if (cnt > 0 && total > 0) {
      goal = t.nn_val[clamped(first + pick_of(t.u_choice[b], cnt), 0, total - 1, bad)];
      if (goal < 0 || goal > top) bad = true;  // (the clip below brings it inside)
    } else {
      goal = rs;  // no neighbour recorded: the reference's fallback
    }
  }
  // the definition's own clip of the goal (PlayIndex.sample): no status
  goal = goal < 0 ? 0 : (goal > t.last_end ? t.last_end : goal);
  if (goal > top) { bad = true; goal = top; }
  {
    long* __restrict__ dst = t.ids + (long)b * Tmax;
    for (int i = lane; i < Tmax; i += 64) dst[i] = s + (i < ws ? i : ws - 1);  // pad by repetition of the last frame
  }
  {
    const float* __restrict__ src = t.actions + s * A;
    float* __restrict__ dst = t.act + (long)b * Tmax * A;
    const int n = ws * A, pad = (Tmax - ws) * A;
    const float grip = src[n - 1];  // the last real step's gripper action
    for (int i = lane; i < n; i += 64) dst[i] = src[i];
    for (int i = lane; i < pad; i += 64) dst[n + i] = (i % A == A - 1) ? grip : 0.f;
  }
  if (lane != 0) return;
  t.ids[(long)B * Tmax + b] = goal;
  t.disp_out[b] = strat == 0 ? d : -1;
  t.window_size[b] = ws;
  if (bad) *t.status = 1;
}

}  // namespace

extern "C" int tacorl_sample_play_windows(const long* episode_lookup, long n_items, const long* ep_start, const long* ep_end,
                                          int n_episodes, const long* nn_ptr, long n_nn, const long* nn_val,
                                          const float* actions, long n_frames, long last_end, const long* idx,
                                          const long* window, const long* strategy, const long* disp, const long* noise_step,
                                          const double* u_choice, const double* u_random_state, int B, int Tmax, int A,
                                          int min_window, long* ids, float* act, long* disp_out, long* window_size,
                                          int* status, tacorl_stream_t stream) {
  if (B <= 0 || Tmax <= 0 || A <= 0 || n_items <= 0 || n_episodes <= 0 || n_frames <= 0 || n_nn < 0) return TACORL_EINVAL;
  if (min_window < 1 || min_window > Tmax || n_frames < Tmax || last_end < 0 || last_end >= n_frames) return TACORL_EINVAL;
  if ((long)Tmax * A > 0x7fffffffL || (long)B + 3 > 0x7fffffffL) return TACORL_EINVAL;
  if (!pointers_ok({episode_lookup, ep_start, ep_end, idx, window, strategy, disp, u_choice, u_random_state, ids, disp_out,
                    window_size}, 8) ||
      !pointers_ok({actions, act, status}, 4) || !pointers_ok({noise_step}, 8, true) ||
      (n_nn > 0 && !pointers_ok({nn_ptr, nn_val}, 8)))
    return TACORL_EINVAL;
  const PlayTbl t{episode_lookup, n_items, ep_start, ep_end, n_episodes, nn_ptr, n_nn, nn_val, actions, n_frames, last_end,
                  idx, window, strategy, disp, noise_step, u_choice, u_random_state, ids, act, disp_out, window_size, status};
  hipLaunchKernelGGL(sample_play_windows_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, t, B, Tmax, A,
                     min_window);
  return LAUNCH_OK();
}

extern "C" int tacorl_sample_d4rl_windows(const long* episode_lookup, long n_items, const long* ep_start, const long* ep_end,
                                          int n_episodes, const float* observations, const float* actions, long n_frames,
                                          const long* idx, const long* window, const long* disp, int B, int Tmax, int S, int A,
                                          int G, int min_window, float threshold, float* obs, float* act, float* goal,
                                          float* reached, float* done, long* window_size, long* ids, int* status,
                                          tacorl_stream_t stream) {
  if (B <= 0 || Tmax <= 0 || S <= 0 || A <= 0 || n_items <= 0 || n_episodes <= 0) return TACORL_EINVAL;
  if (G < 0 || G == 1 || G > S || min_window < 1 || min_window > Tmax || n_frames < Tmax) return TACORL_EINVAL;
  if ((long)Tmax * S > 0x7fffffffL || (long)Tmax * A > 0x7fffffffL || (long)B + 3 > 0x7fffffffL) return TACORL_EINVAL;
  if (!pointers_ok({episode_lookup, ep_start, ep_end, idx, window, disp}, 8) ||
      !pointers_ok({observations, actions, obs, act, status}, 4) || !pointers_ok({goal, reached, done}, 4, true) ||
      !pointers_ok({window_size, ids}, 8, true))
    return TACORL_EINVAL;
  const D4rlTbl t{episode_lookup, n_items, ep_start, ep_end, n_episodes, observations, actions, n_frames, idx, window, disp,
                  obs, act, goal, reached, done, window_size, ids, status};
  hipLaunchKernelGGL(sample_d4rl_windows_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, t, B, Tmax, S, A, G,
                     min_window, threshold);
  return LAUNCH_OK();
}

extern "C" int tacorl_sample_transitions(const long* possible_steps, long n_possible, const long* ep_start,
                                         const long* ep_end, int n_episodes, const long* nn_ptr, long n_nn,
                                         const long* nn_val, const float* actions, const long* idx, const long* strategy,
                                         const long* disp, const double* u_choice, long current_horizon, long n_frames,
                                         int B, int A, long* ids, float* action, float* reward, float* done, int* status,
                                         tacorl_stream_t stream) {
  if (B <= 0 || A <= 0 || n_possible <= 0 || n_episodes <= 0 || n_frames <= 0 || n_nn < 0) return TACORL_EINVAL;
  if (!pointers_ok({possible_steps, ep_start, ep_end, idx, strategy, disp, u_choice, ids}, 8) ||
      !pointers_ok({actions, action, reward, done, status}, 4) || (n_nn > 0 && !pointers_ok({nn_ptr, nn_val}, 8)))
    return TACORL_EINVAL;
  const TransTbl t{possible_steps, n_possible, ep_start, ep_end, n_episodes, nn_ptr, n_nn, nn_val, actions, idx, strategy,
                   disp, u_choice, current_horizon, n_frames, ids, action, reward, done, status};
  hipLaunchKernelGGL(sample_transitions_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, t, B, A);
  return LAUNCH_OK();
}

extern "C" int tacorl_sample_relay(const long* episode_lookup, long n_items, const long* ep_start, const long* ep_end,
                                   int n_episodes, const float* actions, long n_frames, const long* idx, const double* u_low,
                                   const double* u_high, long max_low_level_window, long max_high_level_window, int B, int A,
                                   long* ids, float* action, int* status, tacorl_stream_t stream) {
  if (B <= 0 || A <= 0 || n_items <= 0 || n_episodes <= 0 || n_frames <= 0 || max_low_level_window <= 0 ||
      max_high_level_window <= 0)
    return TACORL_EINVAL;
  if (!pointers_ok({episode_lookup, ep_start, ep_end, idx, u_low, u_high, ids}, 8) || !pointers_ok({actions, action, status}, 4))
    return TACORL_EINVAL;
  const RelayTbl t{episode_lookup, n_items, ep_start, ep_end, n_episodes, actions, n_frames, idx, u_low, u_high,
                   max_low_level_window, max_high_level_window, ids, action, status};
  hipLaunchKernelGGL(sample_relay_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, t, B, A);
  return LAUNCH_OK();
}

extern "C" int tacorl_gather_frames_u8(const void* frames, long frame_bytes, const long* index, void* dst, long n,
                                       tacorl_stream_t stream) {
  if (!frames || !index || !dst || frame_bytes <= 0 || frame_bytes % 16 || ((uintptr_t)frames & 15) || ((uintptr_t)dst & 15))
    return TACORL_EINVAL;
  if (n <= 0) return TACORL_OK;
  const int chunks = (int)(frame_bytes / 16);
  const long blocks = (n * chunks + 255) / 256;
  hipLaunchKernelGGL(gather_frames_u8_kernel, dim3((int)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)frames, frame_bytes, index, (unsigned char*)dst, n, chunks);
  return LAUNCH_OK();
}

extern "C" int tacorl_pack_images_u8_aug_batch(int njobs, const void* const* src, const long* img_pitch_bytes,
                                               void* const* dst, const int* const* shift, const float* const* jitter,
                                               const int* n_img, int dst_dtype, int H, int W, int pad,
                                               tacorl_stream_t stream) {
  return tacorl_pack_images_u8_aug_gather_batch(njobs, src, img_pitch_bytes, nullptr, nullptr, dst, shift, jitter, n_img,
                                                dst_dtype, H, W, pad, stream);
}
extern "C" int tacorl_pack_images_u8_aug_gather_batch(int njobs, const void* const* src, const long* img_pitch_bytes,
                                                      const long* const* index, const int* index_stride,
                                                      void* const* dst, const int* const* shift, const float* const* jitter,
                                                      const int* n_img, int dst_dtype, int H, int W, int pad,
                                                      tacorl_stream_t stream) {
  return tacorl_pack_images_u8_resize_aug_gather_batch(njobs, src, img_pitch_bytes, index, index_stride, dst, shift, jitter,
                                                       n_img, dst_dtype, H, W, H, W, pad, stream);
}
extern "C" int tacorl_pack_images_u8_resize_aug_gather_batch(int njobs, const void* const* src, const long* img_pitch_bytes,
                                                             const long* const* index, const int* index_stride,
                                                             void* const* dst, const int* const* shift,
                                                             const float* const* jitter, const int* n_img, int dst_dtype,
                                                             int src_H, int src_W, int H, int W, int pad,
                                                             tacorl_stream_t stream) {
  const int Hs = src_H, Ws = src_W;
  if (njobs < 1 || njobs > AUG_MAXJ || H < 1 || W < 1 || Hs < 1 || Ws < 1 || pad < 0) return TACORL_EINVAL;
  AugTbl t{};
  int m = 0, mx = 0;
  for (int j = 0; j < njobs; j++) {
    if (n_img[j] <= 0) continue;
    if (!src[j] || !dst[j]) return TACORL_EINVAL;
    const long* ix = index ? index[j] : nullptr;
    const int is = (ix && index_stride) ? index_stride[j] : 1;
    if (ix && is < 1) return TACORL_EINVAL;
    t.j[m] = AugJob{(const unsigned char*)src[j], img_pitch_bytes[j], dst[j], shift ? shift[j] : nullptr,
                    jitter ? jitter[j] : nullptr, ix, is, n_img[j]};
    mx = n_img[j] > mx ? n_img[j] : mx;
    m++;
  }
  if (m == 0) return TACORL_OK;
  if (dst_dtype == TACORL_BF16)
    hipLaunchKernelGGL(pack_u8_aug_kernel<__bf16>, dim3(mx, m), dim3(256), 0, (hipStream_t)stream, t, H, W, pad, Hs, Ws);
  else
    hipLaunchKernelGGL(pack_u8_aug_kernel<float>, dim3(mx, m), dim3(256), 0, (hipStream_t)stream, t, H, W, pad, Hs, Ws);
  return LAUNCH_OK();
}
