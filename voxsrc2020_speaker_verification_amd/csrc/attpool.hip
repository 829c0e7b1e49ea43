// Attentive statistics pooling tail (models.py:273-303): softmax over time of
// the attention logits, weighted mean and std of x, head BN, NHWC flatten
// (feature w*2C + j).  One thread per (n, w, c): coalesced over c, every sum
// sequential in t (a fixed order per column, batch-independent).
//
// Ragged batches (vlen / vsh): utterance n takes its max, sum, mean and std
// over its valid_rows Hn only, in the order an H = Hn launch takes, and never
// reads a row at or past Hn (neither the logits nor x: padding may hold NaN or
// Inf).  A block's 256 threads may span utterances, so Hn is per thread.
//
// Arithmetic per element, pinned so that every variant writes the same bits:
//   e_t = expf(l_t - mx),  sum += e_t,  wt = e_t / sum,
//   wm = fma(x, wt, wm),   wss = fma(x * x, wt, wss),
//   sd = sqrtf(fma(-wm, wm, wss) + eps),  then bn2d.
// The logits of the first RM rows stay in registers from the max pass, their
// e_t from the sum pass: those rows are read once and take one expf (the plain
// form read the logits three times and evaluated expf twice per element);
// rows past RM re-read and re-evaluate, to the same values.
#include <cmath>
#include "kernels.h"
#include "device_common.h"

namespace vox {

template <typename T>
__global__ __launch_bounds__(256) void att_pool_k(const T* __restrict__ x,
                                                  const float* __restrict__ lg, int N, int H,
                                                  int W, int C, float eps,
                                                  const float* __restrict__ mean,
                                                  const float* __restrict__ inv,
                                                  float* __restrict__ out,
                                                  const int* __restrict__ vlen, int vsh) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)N * W * C) return;
  const int c = (int)(i % C);
  const int64_t nw = i / C;
  const int w = (int)(nw % W);
  const int64_t n = nw / W;
  const int Hn = valid_rows(vlen, vsh, (int)n, H);
  const int64_t base = (n * H * W + w) * C + c, st = (int64_t)W * C;
  constexpr int RM = 32;   // rows held in registers (T <= 256 frames: all of them)
  float e[RM];
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < RM; ++t)
    if (t < Hn) {
      e[t] = lg[base + t * st];
      mx = fmaxf(mx, e[t]);
    }
  for (int t = RM; t < Hn; ++t) mx = fmaxf(mx, lg[base + t * st]);
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < RM; ++t)
    if (t < Hn) {
      e[t] = expf(e[t] - mx);
      sum += e[t];
    }
  for (int t = RM; t < Hn; ++t) sum += expf(lg[base + t * st] - mx);
  float wm = 0.f, wss = 0.f;
#pragma unroll
  for (int t = 0; t < RM; ++t)
    if (t < Hn) {
      const float wt = e[t] / sum;
      const float xv = (float)x[base + t * st];
      const float xx = xv * xv;
      wm = __builtin_fmaf(xv, wt, wm);
      wss = __builtin_fmaf(xx, wt, wss);
    }
  for (int t = RM; t < Hn; ++t) {
    const float wt = expf(lg[base + t * st] - mx) / sum;
    const float xv = (float)x[base + t * st];
    const float xx = xv * xv;
    wm = __builtin_fmaf(xv, wt, wm);
    wss = __builtin_fmaf(xx, wt, wss);
  }
  const float sd = sqrtf(__builtin_fmaf(-wm, wm, wss) + eps);
  float* o = out + n * W * 2 * C + (int64_t)w * 2 * C;
  const int j0 = w * 2 * C + c, j1 = j0 + C;
  o[c] = mean ? bn2d(wm, inv[j0], mean[j0]) : wm;
  o[C + c] = mean ? bn2d(sd, inv[j1], mean[j1]) : sd;
}

hipError_t launch_att_pool(DType t, const void* x, const float* lg, int N, int H, int W, int C,
                           float eps, const float* mean, const float* inv, float* out,
                           hipStream_t s, const int* vlen, int vsh) {
  const int64_t total = (int64_t)N * W * C;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (t == BF16)
    hipLaunchKernelGGL((att_pool_k<bf16_t>), grid, dim3(256), 0, s,
                       reinterpret_cast<const bf16_t*>(x), lg, N, H, W, C, eps, mean, inv, out,
                       vlen, vsh);
  else
    hipLaunchKernelGGL((att_pool_k<float>), grid, dim3(256), 0, s,
                       reinterpret_cast<const float*>(x), lg, N, H, W, C, eps, mean, inv, out,
                       vlen, vsh);
  return hipGetLastError();
}

}  // namespace vox
