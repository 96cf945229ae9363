// Store-time resize of the resident replay (dataset key `store_size`): n uint8 HWC camera frames -> n uint8 HWC frames of
// H x W, bilinear with align_corners = False and no antialias on the 0..255 values in fp32 - the sampling rule and the
// four-term sum of bilinear.h, which the Resize stage of the augmenting pack (data_ops.hip) evaluates too - then round to
// nearest even, clamp to 0..255, store.  The loader (tacorl_amd/data/frame_dir.py) passes every uploaded chunk through it,
// so only the chunk buffer ever holds camera-resolution frames on the device.
//
// A streaming kernel: one workgroup per band of RESIZE_BAND output rows of one frame.  The source rows the band samples
// are one contiguous byte range of the source frame; it is staged into the LDS once, with 16-byte loads on 16-byte
// boundaries of the source buffer - the source row pair of an output row is read from memory once (once per band where
// neighbouring output rows share it), however many pixels sample it.  The band's output rows are one contiguous byte range of the destination frame: a thread produces one
// 16-byte chunk on a 16-byte boundary of the destination buffer from the staged rows and stores it with one 16-byte vector
// store.  Bands are 16 rows, so a band's bytes (16 * W * 3) are a multiple of 16: with a frame size and pitch that are
// multiples of 16 (128 x 128, 84 x 84, every size the fused encoder takes) every access is a full 16-byte one.  Otherwise
// the chunks that straddle a frame's first or last byte (destination) or the buffer's last byte (source) are moved byte by
// byte, so that no byte outside the caller's frames is read or written.
// Measured (profiles/frame_dir.md): 2048 frames 200 x 200 -> 128 x 128 in 0.16 ms, 2.1 TB/s read + written = a third of the
// HBM copy rate; a thread recomputes the column weights per pixel and divides once per chunk.  A first load is bound by the
// host's decompression (the kernel is 0.01 % of it), so it is left there.
#include "../../include/tacorl_hip.h"
#include "bilinear.h"
#include "common.h"

#include <cstdint>

namespace {

constexpr int RESIZE_BAND = 16;            // output rows per workgroup
constexpr long RESIZE_LDS_MAX = 48 * 1024; // staged source bytes per band
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct ResizeArgs {
  const unsigned char* src; long src_pitch;  // 16-byte aligned base, bytes between frames
  unsigned char* dst; long dst_pitch;
  long n, src_valid;                         // frames; bytes of the source buffer that hold frames: (n - 1) * pitch + frame
  int Hs, Ws, H, W, bands, max_rows;         // bands per frame; source rows the LDS holds
};

__global__ __launch_bounds__(256) void resize_frames_u8_kernel(ResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rows[];
  const float sch = (float)a.Hs / (float)a.H, scw = (float)a.Ws / (float)a.W;
  const long row_s = (long)a.Ws * 3, row_d = (long)a.W * 3;
  const long work = a.n * a.bands;
  for (long wk = blockIdx.x; wk < work; wk += gridDim.x) {
    const long img = wk / a.bands;
    const int r0 = (int)(wk - img * a.bands) * RESIZE_BAND, r1 = min(r0 + RESIZE_BAND, a.H);
    // the source rows [ya, yb] the band samples (bilinear_axis is monotone in the output row)
    int ya, yb, t0, t1;
    float f0, f1;
    bilinear_axis(r0, sch, a.Hs, ya, t1, f0, f1);
    bilinear_axis(r1 - 1, sch, a.Hs, t0, yb, f0, f1);
    yb = min(yb, ya + a.max_rows - 1);  // (never binds: the host sized the LDS for the band; keeps the staging inside it)
    const long s_beg = img * a.src_pitch + ya * row_s, s_end = img * a.src_pitch + (yb + 1) * row_s;
    const long s_al = s_beg & ~15L;     // the LDS holds source bytes [s_al, s_end) at rows[off - s_al]
    __syncthreads();                    // the previous band's readers are done
    for (long c = s_al + 16L * threadIdx.x; c < s_end; c += 16L * 256) {
      if (c + 16 <= a.src_valid) {
        *reinterpret_cast<u32x4*>(rows + (c - s_al)) = *reinterpret_cast<const u32x4*>(a.src + c);
      } else {
        for (long b = c; b < a.src_valid && b < c + 16; b++) rows[b - s_al] = a.src[b];
      }
    }
    __syncthreads();
    const unsigned char* base = rows + (s_beg - s_al);  // source row ya, pixel 0
    const long f_beg = img * a.dst_pitch;
    const long d_beg = f_beg + r0 * row_d, d_end = f_beg + r1 * row_d;
    // 16-byte chunks on 16-byte boundaries of the destination; of a chunk that straddles the band's first or last byte
    // (a frame that starts or ends off a boundary) this band writes its own bytes [lo, hi) only, bytewise
    for (long c = (d_beg & ~15L) + 16L * threadIdx.x; c < d_end; c += 16L * 256) {
      const long lo = c < d_beg ? d_beg : c, hi = c + 16 < d_end ? c + 16 : d_end;
      u32x4 out = {0u, 0u, 0u, 0u};
      const long o = lo - f_beg;        // byte of the frame: ((y * W) + x) * 3 + ch
      int y = (int)(o / row_d);
      const int rem = (int)(o - y * row_d);
      int x = rem / 3, ch = rem - x * 3;
      int y0, y1, x0, x1;
      float h0, h1, w0, w1;
      bilinear_axis(y, sch, a.Hs, y0, y1, h0, h1);
      bilinear_axis(x, scw, a.Ws, x0, x1, w0, w1);
#pragma unroll
      for (int k = 0; k < 16; k++) {
        const long b = c + k;
        if (b >= lo && b < hi) {
          const unsigned char *q0 = base + (long)(y0 - ya) * row_s, *q1 = base + (long)(y1 - ya) * row_s;
          const float v = bilinear_mix(h0, h1, w0, w1, q0[x0 * 3 + ch], q0[x1 * 3 + ch], q1[x0 * 3 + ch], q1[x1 * 3 + ch]);
          out[k >> 2] |= (unsigned)fminf(fmaxf(rintf(v), 0.f), 255.f) << (8 * (k & 3));  // round to nearest even, clamp
          if (++ch == 3) {
            ch = 0;
            if (++x == a.W) {
              x = 0;
              y++;
              bilinear_axis(min(y, a.H - 1), sch, a.Hs, y0, y1, h0, h1);
            }
            bilinear_axis(x, scw, a.Ws, x0, x1, w0, w1);
          }
        }
      }
      if (lo == c && hi == c + 16) {
        *reinterpret_cast<u32x4*>(a.dst + c) = out;
      } else {
#pragma unroll
        for (int k = 0; k < 16; k++)
          if (c + k >= lo && c + k < hi) a.dst[c + k] = (unsigned char)(out[k >> 2] >> (8 * (k & 3)));
      }
    }
  }
}

}  // namespace

extern "C" int tacorl_resize_frames_u8(const void* src, long src_pitch_bytes, void* dst, long dst_pitch_bytes, long n,
                                       int src_H, int src_W, int H, int W, tacorl_stream_t stream) {
  if (!src || !dst || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return TACORL_EINVAL;
  if (n <= 0 || src_H < 1 || src_W < 1 || H < 1 || W < 1) return TACORL_EINVAL;
  const long row_s = (long)src_W * 3;
  if (src_pitch_bytes < (long)src_H * row_s || dst_pitch_bytes < (long)H * W * 3) return TACORL_EINVAL;
  // the source rows a band of RESIZE_BAND output rows can sample: its first and last row lie scale * (BAND - 1) apart, each
  // reads the row below too, and the fp32 rounding of the two positions is far below one row
  const double scale = (double)src_H / (double)H;
  long max_rows = (long)(scale * (RESIZE_BAND - 1)) + 4;
  if (max_rows > src_H) max_rows = src_H;
  const long lds = max_rows * row_s + 16;  // + the bytes between the 16-byte boundary and the first row
  if (lds > RESIZE_LDS_MAX) return TACORL_EINVAL;
  const int bands = (H + RESIZE_BAND - 1) / RESIZE_BAND;
  const long work = n * bands;
  ResizeArgs a{(const unsigned char*)src, src_pitch_bytes, (unsigned char*)dst, dst_pitch_bytes, n,
               (n - 1) * src_pitch_bytes + (long)src_H * row_s, src_H, src_W, H, W, bands, (int)max_rows};
  hipLaunchKernelGGL(resize_frames_u8_kernel, dim3((unsigned)(work < (1L << 20) ? work : (1L << 20))), dim3(256),
                     (size_t)((lds + 15) & ~15L), (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? TACORL_OK : TACORL_ELAUNCH;
}
