// adamw.hip — AdamW over one contiguous run of a flat parameter bucket (dist.GradReducer keeps fp32 masters, fp32 gradients and the
// 16-bit working copies of a bucket in flat buffers at identical offsets).  Replaces torch.optim.AdamW(fused=True)'s multi-tensor
// launches (config/sod.yml:57-60: AdamW, lr 5e-4, weight_decay 0.1, per-prefix lr multipliers = one run per multiplier), the
// master -> working-copy cast and - in fp16 mode - GradScaler.unscale_/step of the reference's AmpOptimWrapper (config/sod.yml:57),
// in one pass:
//   g *= inv_scale;  p *= 1 - lr*wd;  m += (1-b1)(g - m);  v = b2 v + (1-b2) g^2;  p -= (lr/bc1) m / (sqrt(v)/sqrt(bc2) + eps);  w = half(p)
// (the update order of torch's _fused_adamw); the whole launch is a no-op when *found_inf != 0 (GradScaler skips the step).
// HBM-bound: 28 B/element (+2 with the working copy); 16-byte accesses on the aligned body, scalars on the unaligned head/tail.
// EMA of the weights (mmengine's EMAHook): the averaged copy of the masters lives in a flat buffer at the same offsets and is updated in
// the same pass from the master in registers (+8 B/element: one read, one write), with the coefficient of this step read from device
// memory (dgtd_ema_schedule wrote it), so a captured hipGraph replays the schedule.
#include "common.h"

namespace {

struct AdamArgs { float lr, b1, b2, eps, wd, inv_bc1, inv_sqrt_bc2, log_b1, log_b2; };

__device__ __forceinline__ float adam_one(float p, float g, float& m, float& v, const AdamArgs& a) {
  p *= 1.f - a.lr * a.wd;
  m = m + (1.f - a.b1) * (g - m);
  v = a.b2 * v + (1.f - a.b2) * g * g;
  const float denom = sqrtf(v) * a.inv_sqrt_bc2 + a.eps;
  return p - (a.lr * a.inv_bc1) * (m / denom);
}

enum { CLIP_OFF = 0, CLIP_COEF = 1, CLIP_VALUE = 2 };

// e <- e + c (p - e) over p, e [n]: c == 1 copies (e is not read), c == 0 is the caller's business (it does not call).  Vector accesses on
// [head, head + 4 body4) - both pointers 16-byte aligned there - and a scalar grid-stride loop over the rest (head == n: all of it).
__device__ __forceinline__ void ema_range(const float* __restrict__ p, float* __restrict__ e, int64_t n, int64_t head, float c,
                                          int64_t tid, int64_t nth) {
  const int64_t body4 = (n - head) / 4;
  for (int64_t i = tid; i < body4; i += nth) {
    const int64_t o = head + i * 4;
    f32x4 pv = *reinterpret_cast<const f32x4*>(p + o);
    if (c != 1.f) {
      const f32x4 ev = *reinterpret_cast<const f32x4*>(e + o);
#pragma unroll
      for (int j = 0; j < 4; ++j) pv[j] = ev[j] + c * (pv[j] - ev[j]);
    }
    *reinterpret_cast<f32x4*>(e + o) = pv;
  }
  const int64_t tail0 = head + body4 * 4, nscal = head + (n - tail0);
  for (int64_t t = tid; t < nscal; t += nth) {
    const int64_t o = t < head ? t : tail0 + (t - head);
    const float pj = p[o];
    e[o] = c == 1.f ? pj : e[o] + c * (pj - e[o]);
  }
}

// the un-scaled gradient after clipping: CLIP_COEF multiplies by the global-norm coefficient, CLIP_VALUE clamps to +-c with comparisons
// that let a NaN through (torch's clamp_); CLIP_OFF is the expression the kernel had before clipping existed
template <int CLIP>
__device__ __forceinline__ float clipped(float g, float gs, float c) {
  if (CLIP == CLIP_COEF) return (g * gs) * c;
  if (CLIP == CLIP_VALUE) { const float u = g * gs; return u < -c ? -c : (u > c ? c : u); }
  return g * gs;
}

template <typename WT, int CLIP, bool EMA>
__global__ __launch_bounds__(256) void adamw_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, WT* __restrict__ w, int64_t n, int64_t head,
                                                         AdamArgs a, const float* __restrict__ amp, const float* __restrict__ lr_dev,
                                                         const WT* __restrict__ g16, const float* __restrict__ clip_coef, float clip_value,
                                                         float* __restrict__ ema, const float* __restrict__ ema_coef) {
  // g16 != NULL: the gradient is the 16-bit all-reduce payload itself (same phase as w), g is not read
  // amp = the loss scaler's device state { scale, growth_tracker, 1/scale, found_inf, steps taken } or NULL
  // lr_dev = the learning rate in device memory (a captured hipGraph replays with whatever the schedule wrote there) or NULL
  // CLIP_COEF: clip_coef = the device scalar dgtd_grad_clip_finalize wrote; CLIP_VALUE: clip_value = the bound
  // EMA: ema = the averaged copy of p (same phase), ema_coef = this step's coefficient in device memory (0: ema is left alone)
  float gs = 1.f;
  const float cc = CLIP == CLIP_COEF ? *clip_coef : clip_value;
  const float ec = EMA ? *ema_coef : 0.f;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  if (lr_dev) a.lr = *lr_dev;
  if (amp) {
    if (amp[3] != 0.f) {                                    // overflowed step: parameters, moments and working copies stay as they are
      if (EMA && ec != 0.f) ema_range(p, ema, n, head, ec, tid, nth);   // mmengine's hook runs after every iteration, skipped or not
      return;
    }
    gs = amp[2];
    const float t = amp[4] + 1.f;                           // skipped steps do not advance the bias corrections (GradScaler.step)
    a.inv_bc1 = -1.f / expm1f(t * a.log_b1);
    a.inv_sqrt_bc2 = rsqrtf(-expm1f(t * a.log_b2));
  }
  typedef typename Vec8<WT>::type W4;
  const int64_t body4 = (n - head) / 4;                      // float4 groups after the unaligned head
  for (int64_t i = tid; i < body4; i += nth) {
    const int64_t o = head + i * 4;
    f32x4 pv = *reinterpret_cast<f32x4*>(p + o), mv = *reinterpret_cast<f32x4*>(m + o), vv = *reinterpret_cast<f32x4*>(v + o);
    f32x4 gv;
    if (g16) {
      const W4 hv = *reinterpret_cast<const W4*>(g16 + o);
#pragma unroll
      for (int j = 0; j < 4; ++j) gv[j] = (float)hv[j];
    } else {
      gv = *reinterpret_cast<const f32x4*>(g + o);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { float mj = mv[j], vj = vv[j]; pv[j] = adam_one(pv[j], clipped<CLIP>(gv[j], gs, cc), mj, vj, a); mv[j] = mj; vv[j] = vj; }
    *reinterpret_cast<f32x4*>(p + o) = pv;
    *reinterpret_cast<f32x4*>(m + o) = mv;
    *reinterpret_cast<f32x4*>(v + o) = vv;
    if (w) {
      W4 wv;
#pragma unroll
      for (int j = 0; j < 4; ++j) wv[j] = (WT)pv[j];
      *reinterpret_cast<W4*>(w + o) = wv;
    }
    if (EMA && ec != 0.f) {                                  // uniform: one coefficient for the whole launch
      if (ec != 1.f) {
        const f32x4 ev = *reinterpret_cast<const f32x4*>(ema + o);
#pragma unroll
        for (int j = 0; j < 4; ++j) pv[j] = ev[j] + ec * (pv[j] - ev[j]);
      }
      *reinterpret_cast<f32x4*>(ema + o) = pv;
    }
  }
  // head [0, head) and tail [head + 4*body4, n): at most 6 scalars
  const int64_t tail0 = head + body4 * 4;
  const int64_t nscal = head + (n - tail0);
  if (tid < nscal) {
    const int64_t o = tid < head ? tid : tail0 + (tid - head);
    float mj = m[o], vj = v[o];
    const float pj = adam_one(p[o], clipped<CLIP>(g16 ? (float)g16[o] : g[o], gs, cc), mj, vj, a);
    p[o] = pj; m[o] = mj; v[o] = vj;
    if (w) w[o] = (WT)pj;
    if (EMA && ec != 0.f) ema[o] = ec == 1.f ? pj : ema[o] + ec * (pj - ema[o]);
  }
}

// the EMA update alone (stretches AdamW does not visit, float buffers)
__global__ __launch_bounds__(256) void ema_flat_kernel(const float* __restrict__ p, float* __restrict__ e, int64_t n, int64_t head,
                                                       const float* __restrict__ ema_coef) {
  const float c = *ema_coef;
  if (c == 0.f) return;
  ema_range(p, e, n, head, c, (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256);
}

// p <-> e in place; w (16-bit working copy of p, same phase, or NULL) is rewritten from the new p
template <typename WT>
__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ p, float* __restrict__ e, WT* __restrict__ w, int64_t n, int64_t head) {
  typedef typename Vec8<WT>::type W4;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  const int64_t body4 = (n - head) / 4;
  for (int64_t i = tid; i < body4; i += nth) {
    const int64_t o = head + i * 4;
    const f32x4 pv = *reinterpret_cast<const f32x4*>(p + o), ev = *reinterpret_cast<const f32x4*>(e + o);
    *reinterpret_cast<f32x4*>(p + o) = ev;
    *reinterpret_cast<f32x4*>(e + o) = pv;
    if (w) {
      W4 wv;
#pragma unroll
      for (int j = 0; j < 4; ++j) wv[j] = (WT)ev[j];
      *reinterpret_cast<W4*>(w + o) = wv;
    }
  }
  const int64_t tail0 = head + body4 * 4, nscal = head + (n - tail0);
  for (int64_t t = tid; t < nscal; t += nth) {
    const int64_t o = t < head ? t : tail0 + (t - head);
    const float pj = p[o], ej = e[o];
    p[o] = ej; e[o] = pj;
    if (w) w[o] = (WT)ej;
  }
}

// mmengine's EMAHook / BaseAveragedModel schedule on the device: state = { coef of this step, steps (updates counted), iters seen, enabled }.
__global__ void ema_schedule_kernel(float* __restrict__ state, int kind, float momentum, float gamma, int interval, int begin_iter) {
  float coef = 1.f, steps = state[1];                       // before begin_iter / while disabled the average is a copy of the weights
  const float iters = state[2];
  if (state[3] != 0.f && iters >= (float)begin_iter) {
    const int k = (int)steps;
    if (k == 0) coef = 1.f;
    else if (k % interval != 0) coef = 0.f;
    else if (kind == 0) coef = momentum;
    else if (kind == 1) coef = fmaxf(momentum, (float)((double)gamma / ((double)gamma + (double)k)));
    else coef = (float)(1.0 / (double)(k / interval + 1));
    steps += 1.f;
  }
  state[0] = coef; state[1] = steps; state[2] = iters + 1.f;
}

// found[0] = 1 if any element of g[0, n) is inf or NaN (left untouched otherwise): the `found_inf` of GradScaler.unscale_.
__global__ __launch_bounds__(256) void found_inf_kernel(const float* __restrict__ g, int64_t n, int64_t head, float* __restrict__ found) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  const int64_t body4 = (n - head) / 4;
  bool bad = false;
  for (int64_t i = tid; i < body4; i += nth) {
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + head + i * 4);
    // x - x is 0 for every finite x and NaN for inf / NaN
    const float t = (gv[0] - gv[0]) + (gv[1] - gv[1]) + (gv[2] - gv[2]) + (gv[3] - gv[3]);
    bad |= !(t == 0.f);
  }
  const int64_t tail0 = head + body4 * 4, nscal = head + (n - tail0);
  if (tid < nscal) { const float x = g[tid < head ? tid : tail0 + (tid - head)]; bad |= !((x - x) == 0.f); }
  if (__any(bad) && (threadIdx.x & 63) == 0) *found = 1.f;   // same value from every writer: no atomic needed
}

// ---- global gradient norm (clip_grad of the reference's optim_wrapper): per-workgroup fp64 partials, then one finalize --------------
enum { NORM_L2 = 0, NORM_INF = 1 };

// L2: a + x^2, every element widened to fp64 first (fp32 squares overflow from |g| ~ 1.8e19; max_f32^2 fits fp64, so the sum is
// non-finite iff an element is).  inf: max(a, |x|) that keeps a NaN from either side.
template <int KIND>
__device__ __forceinline__ double norm_acc(double a, double x) {
  if (KIND == NORM_L2) return a + x * x;
  const double ax = fabs(x);
  return (ax > a || ax != ax) ? ax : a;
}
template <int KIND>
__device__ __forceinline__ double norm_merge(double a, double b) {
  if (KIND == NORM_L2) return a + b;
  return (b > a || b != b) ? b : a;
}

// fixed order: the 64 lanes of a wave by halving strides, then the waves of the workgroup in index order through LDS; thread 0 returns
template <int KIND, int WAVES>
__device__ __forceinline__ double norm_block_reduce(double acc) {
  __shared__ double red[WAVES];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc = norm_merge<KIND>(acc, __shfl_down(acc, off));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  double r = red[0];
  if (threadIdx.x == 0) for (int i = 1; i < WAVES; ++i) r = norm_merge<KIND>(r, red[i]);
  return r;
}

// partial[blockIdx.x] = sum of squares / max magnitude of this workgroup's grid-stride share of g[0, n).  16-byte loads on the aligned
// body (four in flight per lane, each with its own accumulator), scalars on the unaligned head / tail.  No atomics: the result is
// a function of (n, head, grid) alone.
template <typename T, int KIND>
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const T* __restrict__ g, int64_t n, int64_t head, double* __restrict__ partial) {
  typedef typename Vec16<T>::type V;
  constexpr int N = Vec16<T>::N;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  const int64_t body = (n - head) / N;                       // 16-byte groups after the unaligned head
  const V* __restrict__ gb = reinterpret_cast<const V*>(g + head);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int64_t i = tid;
  for (; i + 3 * nth < body; i += 4 * nth) {
    const V v0 = gb[i], v1 = gb[i + nth], v2 = gb[i + 2 * nth], v3 = gb[i + 3 * nth];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      a0 = norm_acc<KIND>(a0, (double)(float)v0[j]);
      a1 = norm_acc<KIND>(a1, (double)(float)v1[j]);
      a2 = norm_acc<KIND>(a2, (double)(float)v2[j]);
      a3 = norm_acc<KIND>(a3, (double)(float)v3[j]);
    }
  }
  for (; i < body; i += nth) {
    const V v0 = gb[i];
#pragma unroll
    for (int j = 0; j < N; ++j) a0 = norm_acc<KIND>(a0, (double)(float)v0[j]);
  }
  // head [0, head) and tail [head + N*body, n): at most 2 (N - 1) scalars
  const int64_t tail0 = head + body * N, nscal = head + (n - tail0);
  if (tid < nscal) a1 = norm_acc<KIND>(a1, (double)(float)g[tid < head ? tid : tail0 + (tid - head)]);
  const double r = norm_block_reduce<KIND, 4>(norm_merge<KIND>(norm_merge<KIND>(a0, a1), norm_merge<KIND>(a2, a3)));
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// One workgroup: every partial of every bucket in index order -> total norm (x 1/scale) rounded ONCE to fp32 -> clip coefficient.
template <int KIND>
__global__ __launch_bounds__(1024) void grad_clip_finalize_kernel(const double* __restrict__ partials, int64_t count, float max_norm,
                                                                  float* __restrict__ amp, float* __restrict__ clip_state) {
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 1024) acc = norm_merge<KIND>(acc, partials[i]);
  const double s = norm_block_reduce<KIND, 16>(acc);
  if (threadIdx.x != 0) return;
  double t = KIND == NORM_L2 ? sqrt(s) : s;
  if (amp) {
    t *= (double)amp[2];
    if (!(s - s == 0.0)) amp[3] = 1.f;                       // an inf / NaN gradient: this write is the step's found_inf
  }
  const float total = (float)t;
  const float coef = max_norm / (total + 1e-6f);             // torch.nn.utils.clip_grad_norm_; a NaN stays a NaN through the clamp
  clip_state[0] = total;
  clip_state[1] = coef > 1.f ? 1.f : coef;
}

// GradScaler.update() (torch/amp/grad_scaler.py _amp_update_scale_): state = { scale, growth_tracker, inv_scale, found_inf, steps }.
__global__ void loss_scale_update_kernel(float* __restrict__ state, float growth, float backoff, int interval) {
  float scale = state[0], tracker = state[1];
  if (state[3] != 0.f) { scale *= backoff; tracker = 0.f; }
  else {
    state[4] += 1.f;                                        // optimizer steps actually taken
    tracker += 1.f;
    if (tracker >= (float)interval) { const float grown = scale * growth; if (grown - grown == 0.f) scale = grown; tracker = 0.f; }
  }
  state[0] = scale; state[1] = tracker; state[2] = 1.f / scale; state[3] = 0.f;
}

}  // namespace

template <typename WT, bool EMA>
static void adamw_launch(int clip, int grid, hipStream_t st, float* p, const float* g, float* m, float* v, WT* w, int64_t n, int64_t head, AdamArgs a,
                         const float* amp, const float* lr_dev, const WT* g16, const float* clip_coef, float clip_value, float* ema, const float* ema_coef) {
  if (clip == CLIP_COEF) hipLaunchKernelGGL((adamw_flat_kernel<WT, CLIP_COEF, EMA>), dim3(grid), dim3(256), 0, st, p, g, m, v, w, n, head, a, amp, lr_dev, g16, clip_coef, clip_value, ema, ema_coef);
  else if (clip == CLIP_VALUE) hipLaunchKernelGGL((adamw_flat_kernel<WT, CLIP_VALUE, EMA>), dim3(grid), dim3(256), 0, st, p, g, m, v, w, n, head, a, amp, lr_dev, g16, clip_coef, clip_value, ema, ema_coef);
  else hipLaunchKernelGGL((adamw_flat_kernel<WT, CLIP_OFF, EMA>), dim3(grid), dim3(256), 0, st, p, g, m, v, w, n, head, a, amp, lr_dev, g16, clip_coef, clip_value, ema, ema_coef);
}

static int adamw_impl(float* p, const float* g, const void* g16, float* m, float* v, void* w, dgtd_dtype w_dt, int64_t n, float lr, float beta1,
                      float beta2, float eps, float weight_decay, float bias_correction1, float bias_correction2,
                      const float* amp_state, const float* lr_dev, const float* clip_coef_dev, float clip_value, float* ema,
                      const float* ema_coef_dev, dgtd_stream s) {
  const int clip = clip_coef_dev ? CLIP_COEF : (clip_value > 0.f ? CLIP_VALUE : CLIP_OFF);
  DGTD_PROF(s, DGTD_HBM, (w ? 30.0 : 28.0) * n - (g16 ? 2.0 * n : 0.0) + (ema ? 8.0 * n : 0.0), "dgtd_adamw_flat[n=%lld%s%s%s]", (long long)n,
            g16 ? ",g16" : "", clip == CLIP_COEF ? ",clip=norm" : (clip == CLIP_VALUE ? ",clip=value" : ""), ema ? ",ema" : "");
  DGTD_REQUIRE(n > 0 && p && (g || g16) && m && v, "adamw_flat: bad arguments");
  DGTD_REQUIRE(!(clip_coef_dev && clip_value > 0.f), "adamw_flat: clip by norm (clip_coef_dev) and by value (clip_value > 0) exclude each other");
  if (!g) g = p;                                                             // never read; keeps the phase checks below trivially true
  DGTD_REQUIRE(!g16 || (DGTD_IS_HALF(w_dt) && ((uintptr_t)g16 % 8) * 2 == (uintptr_t)p % 16), "adamw_flat: the 16-bit gradient must share the phase of the masters");
  DGTD_REQUIRE(amp_state || (bias_correction1 > 0.f && bias_correction2 > 0.f), "adamw_flat: bias corrections must be positive");
  DGTD_REQUIRE(!w || DGTD_IS_HALF(w_dt), "adamw_flat: the working copy is bf16 or fp16, got dtype %d", (int)w_dt);
  const uintptr_t ap = (uintptr_t)p;
  DGTD_REQUIRE(((uintptr_t)g - ap) % 16 == 0 && ((uintptr_t)m - ap) % 16 == 0 && ((uintptr_t)v - ap) % 16 == 0 && ap % 4 == 0,
               "adamw_flat: p, g, m, v must share their 16-byte phase");
  DGTD_REQUIRE(!w || (((uintptr_t)w % 8) * 2 == ap % 16), "adamw_flat: the working copy must share the phase of the masters");
  DGTD_REQUIRE(!ema || (ema_coef_dev && ((uintptr_t)ema - ap) % 16 == 0), "adamw_flat: the average needs its coefficient and must share the phase of the masters");
  const int64_t head = std::min<int64_t>(n, ((16 - (int64_t)(ap % 16)) % 16) / 4);
  AdamArgs a{lr, beta1, beta2, eps, weight_decay, 1.f / bias_correction1, 1.f / sqrtf(bias_correction2), (float)log((double)beta1), (float)log((double)beta2)};
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv((n + 3) / 4 + 8, 256), 8192));
  if (ema) DGTD_DISPATCH_HALF(w_dt, (adamw_launch<T_, true>(clip, grid, (hipStream_t)s, p, g, m, v, (T_*)w, n, head, a, amp_state, lr_dev, (const T_*)g16, clip_coef_dev, clip_value, ema, ema_coef_dev)));
  else DGTD_DISPATCH_HALF(w_dt, (adamw_launch<T_, false>(clip, grid, (hipStream_t)s, p, g, m, v, (T_*)w, n, head, a, amp_state, lr_dev, (const T_*)g16, clip_coef_dev, clip_value, nullptr, nullptr)));
  DGTD_CHECK_LAUNCH("adamw_flat");
  return 0;
}

extern "C" int dgtd_adamw_flat_amp(float* p, const float* g, float* m, float* v, void* w, dgtd_dtype w_dt, int64_t n, float lr, float beta1,
                                   float beta2, float eps, float weight_decay, float bias_correction1, float bias_correction2,
                                   const float* amp_state, const float* lr_dev, dgtd_stream s) {
  DGTD_REQUIRE(g, "adamw_flat: bad arguments");
  return adamw_impl(p, g, nullptr, m, v, w, w_dt, n, lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2, amp_state, lr_dev, nullptr, 0.f, nullptr, nullptr, s);
}

extern "C" int dgtd_adamw_flat_g16(float* p, const void* g16, float* m, float* v, void* w, dgtd_dtype w_dt, int64_t n, float lr, float beta1,
                                   float beta2, float eps, float weight_decay, float bias_correction1, float bias_correction2,
                                   const float* amp_state, const float* lr_dev, dgtd_stream s) {
  DGTD_REQUIRE(g16, "adamw_flat_g16: bad arguments");
  return adamw_impl(p, nullptr, g16, m, v, w, w_dt, n, lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2, amp_state, lr_dev, nullptr, 0.f, nullptr, nullptr, s);
}

extern "C" int dgtd_adamw_flat(float* p, const float* g, float* m, float* v, void* w_bf16, int64_t n, float lr, float beta1, float beta2,
                               float eps, float weight_decay, float bias_correction1, float bias_correction2, dgtd_stream s) {
  return dgtd_adamw_flat_amp(p, g, m, v, w_bf16, DGTD_BF16, n, lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2,
                             nullptr, nullptr, s);
}

extern "C" int dgtd_adamw_flat_clip(float* p, const float* g, const void* g16, float* m, float* v, void* w, dgtd_dtype w_dt, int64_t n, float lr,
                                    float beta1, float beta2, float eps, float weight_decay, float bias_correction1, float bias_correction2,
                                    const float* amp_state, const float* lr_dev, const float* clip_coef_dev, float clip_value, dgtd_stream s) {
  DGTD_REQUIRE((g != nullptr) != (g16 != nullptr), "adamw_flat_clip: exactly one of g (fp32) and g16 (16-bit payload) is given");
  return adamw_impl(p, g, g16, m, v, w, w_dt, n, lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2, amp_state, lr_dev,
                    clip_coef_dev, clip_value, nullptr, nullptr, s);
}

extern "C" int dgtd_adamw_flat_ema(float* p, const float* g, const void* g16, float* m, float* v, void* w, dgtd_dtype w_dt, int64_t n, float lr,
                                   float beta1, float beta2, float eps, float weight_decay, float bias_correction1, float bias_correction2,
                                   const float* amp_state, const float* lr_dev, const float* clip_coef_dev, float clip_value, float* ema,
                                   const float* ema_coef_dev, dgtd_stream s) {
  DGTD_REQUIRE((g != nullptr) != (g16 != nullptr), "adamw_flat_ema: exactly one of g (fp32) and g16 (16-bit payload) is given");
  return adamw_impl(p, g, g16, m, v, w, w_dt, n, lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2, amp_state, lr_dev,
                    clip_coef_dev, clip_value, ema, ema ? ema_coef_dev : nullptr, s);
}

// head of the 16-byte body shared by p and e, or n (everything scalar) when their phases differ
static int64_t ema_head(const float* p, const float* e, int64_t n) {
  const uintptr_t ap = (uintptr_t)p;
  if (((uintptr_t)e - ap) % 16 != 0) return n;
  return std::min<int64_t>(n, ((16 - (int64_t)(ap % 16)) % 16) / 4);
}

extern "C" int dgtd_ema_flat(const float* p, float* ema, int64_t n, const float* ema_coef_dev, dgtd_stream s) {
  DGTD_PROF(s, DGTD_HBM, 12.0 * n, "dgtd_ema_flat[n=%lld]", (long long)n);
  DGTD_REQUIRE(n > 0 && p && ema && ema_coef_dev, "ema_flat: bad arguments");
  DGTD_REQUIRE((uintptr_t)p % 4 == 0 && (uintptr_t)ema % 4 == 0, "ema_flat: p and ema must be 4-byte aligned");
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv((n + 3) / 4 + 8, 256), 8192));
  hipLaunchKernelGGL(ema_flat_kernel, dim3(grid), dim3(256), 0, (hipStream_t)s, p, ema, n, ema_head(p, ema, n), ema_coef_dev);
  DGTD_CHECK_LAUNCH("ema_flat");
  return 0;
}

template <typename WT>
static void ema_swap_launch(int grid, hipStream_t st, float* p, float* ema, void* w, int64_t n, int64_t head) {
  hipLaunchKernelGGL(ema_swap_kernel<WT>, dim3(grid), dim3(256), 0, st, p, ema, (WT*)w, n, head);
}

extern "C" int dgtd_ema_swap(float* p, float* ema, void* w, dgtd_dtype w_dt, int64_t n, dgtd_stream s) {
  DGTD_PROF(s, DGTD_HBM, (w ? 18.0 : 16.0) * n, "dgtd_ema_swap[n=%lld]", (long long)n);
  DGTD_REQUIRE(n > 0 && p && ema && p != ema, "ema_swap: bad arguments");
  DGTD_REQUIRE((uintptr_t)p % 4 == 0 && (uintptr_t)ema % 4 == 0, "ema_swap: p and ema must be 4-byte aligned");
  DGTD_REQUIRE(!w || DGTD_IS_HALF(w_dt), "ema_swap: the working copy is bf16 or fp16, got dtype %d", (int)w_dt);
  DGTD_REQUIRE(!w || (((uintptr_t)ema - (uintptr_t)p) % 16 == 0 && ((uintptr_t)w % 8) * 2 == (uintptr_t)p % 16),
               "ema_swap: with a working copy p, ema and w must share their 16-byte phase");
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv((n + 3) / 4 + 8, 256), 8192));
  DGTD_DISPATCH_HALF(w_dt, ema_swap_launch<T_>(grid, (hipStream_t)s, p, ema, w, n, ema_head(p, ema, n)));
  DGTD_CHECK_LAUNCH("ema_swap");
  return 0;
}

extern "C" int dgtd_ema_schedule(float* ema_state, int kind, float momentum, float gamma, int interval, int begin_iter, dgtd_stream s) {
  DGTD_REQUIRE(ema_state && kind >= 0 && kind <= 2 && momentum > 0.f && momentum < 1.f && gamma > 0.f && interval >= 1 && begin_iter >= 0,
               "ema_schedule: bad arguments");
  hipLaunchKernelGGL(ema_schedule_kernel, dim3(1), dim3(1), 0, (hipStream_t)s, ema_state, kind, momentum, gamma, interval, begin_iter);
  DGTD_CHECK_LAUNCH("ema_schedule");
  return 0;
}

template <typename T>
static void norm_partial_launch(int kind, int grid, hipStream_t st, const void* g, int64_t n, int64_t head, double* partial) {
  if (kind == NORM_INF) hipLaunchKernelGGL((grad_norm_partial_kernel<T, NORM_INF>), dim3(grid), dim3(256), 0, st, (const T*)g, n, head, partial);
  else hipLaunchKernelGGL((grad_norm_partial_kernel<T, NORM_L2>), dim3(grid), dim3(256), 0, st, (const T*)g, n, head, partial);
}

extern "C" int dgtd_grad_norm_partial(const void* g, dgtd_dtype dt, int64_t n, int kind, double* partial, int grid, dgtd_stream s) {
  DGTD_PROF(s, DGTD_HBM, (dt == DGTD_F32 ? 4.0 : 2.0) * n, "dgtd_grad_norm_partial[n=%lld,%s]", (long long)n, kind == NORM_INF ? "inf" : "l2");
  DGTD_REQUIRE(n > 0 && g && partial && grid >= 1 && grid <= 65535, "grad_norm_partial: bad arguments");
  DGTD_REQUIRE(kind == NORM_L2 || kind == NORM_INF, "grad_norm_partial: kind is 0 (L2) or 1 (inf), got %d", kind);
  DGTD_REQUIRE(dt == DGTD_F32 || DGTD_IS_HALF(dt), "grad_norm_partial: gradients are fp32, bf16 or fp16, got dtype %d", (int)dt);
  const int64_t esz = dt == DGTD_F32 ? 4 : 2;
  const uintptr_t ap = (uintptr_t)g;
  DGTD_REQUIRE(ap % esz == 0 && (uintptr_t)partial % 8 == 0, "grad_norm_partial: g and partial must be aligned to their element size");
  const int64_t head = std::min<int64_t>(n, ((16 - (int64_t)(ap % 16)) % 16) / esz);
  DGTD_DISPATCH(dt, norm_partial_launch<T_>(kind, grid, (hipStream_t)s, g, n, head, partial));
  DGTD_CHECK_LAUNCH("grad_norm_partial");
  return 0;
}

extern "C" int dgtd_grad_clip_finalize(const double* partials, int64_t count, int kind, float max_norm, float* amp_state, float* clip_state,
                                       dgtd_stream s) {
  DGTD_PROF(s, DGTD_HBM, 8.0 * count, "dgtd_grad_clip_finalize[count=%lld]", (long long)count);
  DGTD_REQUIRE(partials && count > 0 && clip_state && max_norm > 0.f, "grad_clip_finalize: bad arguments");
  DGTD_REQUIRE(kind == NORM_L2 || kind == NORM_INF, "grad_clip_finalize: kind is 0 (L2) or 1 (inf), got %d", kind);
  if (kind == NORM_INF) hipLaunchKernelGGL(grad_clip_finalize_kernel<NORM_INF>, dim3(1), dim3(1024), 0, (hipStream_t)s, partials, count, max_norm, amp_state, clip_state);
  else hipLaunchKernelGGL(grad_clip_finalize_kernel<NORM_L2>, dim3(1), dim3(1024), 0, (hipStream_t)s, partials, count, max_norm, amp_state, clip_state);
  DGTD_CHECK_LAUNCH("grad_clip_finalize");
  return 0;
}

extern "C" int dgtd_found_inf(const float* g, int64_t n, float* found, dgtd_stream s) {
  DGTD_PROF(s, DGTD_HBM, 4.0 * n, "dgtd_found_inf[n=%lld]", (long long)n);
  DGTD_REQUIRE(n > 0 && g && found, "found_inf: bad arguments");
  const uintptr_t ap = (uintptr_t)g;
  DGTD_REQUIRE(ap % 4 == 0, "found_inf: g must be 4-byte aligned");
  const int64_t head = std::min<int64_t>(n, ((16 - (int64_t)(ap % 16)) % 16) / 4);
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv((n + 3) / 4 + 8, 256), 4096));
  hipLaunchKernelGGL(found_inf_kernel, dim3(grid), dim3(256), 0, (hipStream_t)s, g, n, head, found);
  DGTD_CHECK_LAUNCH("found_inf");
  return 0;
}

extern "C" int dgtd_loss_scale_update(float* state, float growth_factor, float backoff_factor, int growth_interval, dgtd_stream s) {
  DGTD_REQUIRE(state && growth_factor >= 1.f && backoff_factor > 0.f && backoff_factor <= 1.f && growth_interval > 0, "loss_scale_update: bad arguments");
  hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(1), 0, (hipStream_t)s, state, growth_factor, backoff_factor, growth_interval);
  DGTD_CHECK_LAUNCH("loss_scale_update");
  return 0;
}
