// Error of the three fp32 device functions the noise kernel's normal draw uses (csrc/noise_ops.hip), against fp64, over the
// kernel's WHOLE domain: logf on u1 = m 2^-24 (m = 1 .. 2^24), sqrtf on t = -2 logf(u1) for the same m, sincospif on
// x = m 2^-23 (m = 0 .. 2^24 - 1).  Prints, per function, the largest relative error in units of 2^-23 (an error of N ULP is
// at most N of these units).  tests/noise_ref.py takes its per-function figures from this program's output, recorded in
// profiles/device_noise.md.   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/noise_math_probe.hip -o noise_math_probe
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

__device__ unsigned long long g_max[4];  // bit patterns of non-negative doubles: ordered like the doubles themselves

__device__ double rel_units(float got, double want) {
  if (want == 0.0) return got == 0.0f ? 0.0 : 1e30;
  return fabs(((double)got - want) / want) * 8388608.0;
}

__global__ __launch_bounds__(256) void probe(unsigned n) {
  double e[4] = {0.0, 0.0, 0.0, 0.0};
  for (unsigned m = blockIdx.x * blockDim.x + threadIdx.x; m < n; m += gridDim.x * blockDim.x) {
    const float u1 = (float)(m + 1u) * 0x1p-24f;
    const float l = logf(u1);
    e[0] = fmax(e[0], rel_units(l, log((double)u1)));
    const float t = -2.0f * l;
    e[1] = fmax(e[1], rel_units(sqrtf(t), sqrt((double)t)));
    const float x = (float)m * 0x1p-23f;
    float s, c;
    sincospif(x, &s, &c);
    double sd, cd;
    sincospi((double)x, &sd, &cd);
    e[2] = fmax(e[2], rel_units(s, sd));
    e[3] = fmax(e[3], rel_units(c, cd));
  }
  for (int i = 0; i < 4; i++) atomicMax(&g_max[i], (unsigned long long)__double_as_longlong(e[i]));
}

int main() {
  unsigned long long zero[4] = {0, 0, 0, 0}, out[4];
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_max), zero, sizeof(zero)) != hipSuccess) return 2;
  hipLaunchKernelGGL(probe, dim3(1024), dim3(256), 0, 0, 1u << 24);
  if (hipDeviceSynchronize() != hipSuccess) return 3;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_max), sizeof(out)) != hipSuccess) return 4;
  const char* names[4] = {"logf", "sqrtf", "sincospif.sin", "sincospif.cos"};
  for (int i = 0; i < 4; i++) {
    double d;
    memcpy(&d, &out[i], sizeof(d));
    printf("%-14s max relative error = %.4f x 2^-23\n", names[i], d);
  }
  return 0;
}
