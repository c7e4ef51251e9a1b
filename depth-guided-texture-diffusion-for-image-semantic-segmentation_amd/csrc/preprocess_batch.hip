// preprocess_batch.hip — the reference's input pipeline on the device (twig/dataset/sod_train.py:31-54, :65-83):
// RandomHorizontalFlip -> Resize((S,S)) -> ToTensor (-> Normalize) for uint8 HWC planes already resident in HBM.  ONE pipeline, TWO
// entries: dgtd_preprocess_batch takes a device table of job descriptors (include/dgtd.h: offsets only, never pointers) for a whole
// batch of decoded images of differing sizes and writes input [B,3,S,S], label [B,1,S,S] and depth [B,1,S,S] in place;
// dgtd_preprocess takes one image and builds its one job on the host.  Either way it is THREE launches: the coefficient tables of
// both axes, the horizontal pass, the vertical pass with ToTensor (+ Normalize).  The three device bodies below take a job and the
// base pointers; the batch kernels hand them jobs[blockIdx.y] (blockIdx.x strides over the job's elements, so a small plane simply
// retires most of its blocks at once), the single-image kernels the job they received by value as a kernel argument.
// Resize = Pillow's ImagingResample (BILINEAR, antialiased): triangle filter stretched by the down-scale factor, coefficients
// normalised in double and converted to 22-bit fixed point, horizontal pass then vertical pass with a rounded uint8 intermediate.
// Bit-exact against Pillow / the numpy restatement in oracle/preprocess_cpu.py: the coefficients are Pillow's (IEEE double, every
// operation rounds: this file is compiled with contraction off), the two passes are int32 fixed-point sums in tap order, and
// ToTensor/Normalize is (v/255 - mean)/std in float32, in that order.  Thread -> element map: the horizontal pass gives a thread one
// (row, column, channel) with the channel fastest, so a wave's byte stores are contiguous; the vertical pass gives a thread one
// (channel, row, column) with the column fastest, so the output stores are contiguous.
// Byte work, HBM/latency-bound: sum(H*W*C) bytes in, C*S*S elements out per plane.
#include "common.h"

namespace {

constexpr int PBITS = 32 - 8 - 2;

// 2 * ceil(max(in/out, 1)) + 1.  The double quotient of two int32 is never within an ulp of an integer it does not equal, so the
// integer ceiling IS Pillow's (int)ceil(support); host, device and the Python layout helper all use this form.
__host__ __device__ __forceinline__ int ksize_for(int in_size, int out_size) {
  return (in_size <= out_size ? 1 : (in_size + out_size - 1) / out_size) * 2 + 1;
}

// tables of one job, both axes: thread t < 2S owns output index t % S of axis t / S (0: horizontal from W, 1: vertical from H)
__device__ __forceinline__ void coeffs_body(const dgtd_preprocess_job& jb, char* __restrict__ ws, int S) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * S) return;
  const int axis = t / S, xx = t - axis * S;
  const int in_size = axis ? jb.H : jb.W, out_size = S;
  const int ksize = ksize_for(in_size, out_size);
  int* bounds = (int*)(ws + (axis ? jb.tab_v_off : jb.tab_h_off));
  int* kk = bounds + 2 * (size_t)S;
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const double ss = 1.0 / filterscale;
  const double center = ((double)xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  if (xmax > ksize) xmax = ksize;   // never taken (Pillow sizes ksize for the widest window); keeps the writes inside the table
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) {
    double a = ((double)(x + xmin) - center + 0.5) * ss;
    a = a < 0.0 ? -a : a;
    ww += a < 1.0 ? 1.0 - a : 0.0;
  }
  int* k = kk + (size_t)xx * ksize;
  for (int x = 0; x < ksize; ++x) {
    int v = 0;
    if (x < xmax) {
      double a = ((double)(x + xmin) - center + 0.5) * ss;
      a = a < 0.0 ? -a : a;
      double w = a < 1.0 ? 1.0 - a : 0.0;
      if (ww != 0.0) w = w / ww;
      v = w < 0.0 ? (int)(-0.5 + w * (double)(1 << PBITS)) : (int)(0.5 + w * (double)(1 << PBITS));
    }
    k[x] = v;
  }
  bounds[2 * xx] = xmin;
  bounds[2 * xx + 1] = xmax;
}

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> PBITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// horizontal pass of one job: plane [H][W][C] -> mid [H][S][C]; the flip mirrors the INPUT columns (flip happens before the resize)
__device__ __forceinline__ void resize_h_body(const dgtd_preprocess_job& jb, const uint8_t* __restrict__ planes, char* __restrict__ ws, int S) {
  const int H = jb.H, W = jb.W, C = jb.C, flip = jb.flip;
  const int ksize = ksize_for(W, S);
  const uint8_t* in = planes + jb.src_off;
  uint8_t* mid = (uint8_t*)(ws + jb.mid_off);
  const int* bounds = (const int*)(ws + jb.tab_h_off);
  const int* kk = bounds + 2 * (size_t)S;
  const int64_t total = (int64_t)H * S * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int64_t p = i / C;
    const int xx = (int)(p % S), y = (int)(p / S);
    const int xmin = bounds[2 * xx], cnt = bounds[2 * xx + 1];
    const int* k = kk + (size_t)xx * ksize;
    const uint8_t* row = in + (size_t)y * W * C;
    int acc = 1 << (PBITS - 1);
    for (int x = 0; x < cnt; ++x) {
      const int sx = flip ? W - 1 - (xmin + x) : xmin + x;
      acc += (int)row[(size_t)sx * C + c] * k[x];
    }
    mid[i] = (uint8_t)clip8(acc);   // i == (y * S + xx) * C + c
  }
}

// four pairs: the single-image entry takes C up to 4; the batch entry (C = 3 only where it normalizes) fills the fourth with 0/1
struct NormArgs { float mean[4], stdv[4]; };

// vertical pass + ToTensor (+ Normalize) of one job: mid [H][S][C] -> out_sel[batch][C][S][S]
template <typename T>
__device__ __forceinline__ void resize_v_norm_body(const dgtd_preprocess_job& jb, const char* __restrict__ ws, T* __restrict__ out_input,
                                                   T* __restrict__ out_label, T* __restrict__ out_depth, int S, const NormArgs& na) {
#pragma clang fp contract(off)
  const int C = jb.C;
  const int ksize = ksize_for(jb.H, S);
  const uint8_t* mid = (const uint8_t*)(ws + jb.mid_off);
  const int* bounds = (const int*)(ws + jb.tab_v_off);
  const int* kk = bounds + 2 * (size_t)S;
  T* out = (jb.out_sel == 0 ? out_input : (jb.out_sel == 1 ? out_label : out_depth)) + (size_t)jb.batch * C * S * S;
  const int64_t plane = (int64_t)S * S, total = plane * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i / plane);
    const int64_t p = i - (int64_t)c * plane;
    const int xx = (int)(p % S), yy = (int)(p / S);
    const int ymin = bounds[2 * yy], cnt = bounds[2 * yy + 1];
    const int* k = kk + (size_t)yy * ksize;
    int acc = 1 << (PBITS - 1);
    for (int y = 0; y < cnt; ++y) acc += (int)mid[((size_t)(ymin + y) * S + xx) * C + c] * k[y];
    float t = (float)clip8(acc) / 255.0f;
    if (jb.normalize) {   // compare-and-select on the two bits of c < 4, not an index: a kernel-argument array indexed at run time
                          // goes through scratch, and a chain of three c == k tests is compiled to branches instead of selects
      const float m = (c & 1) ? ((c & 2) ? na.mean[3] : na.mean[1]) : ((c & 2) ? na.mean[2] : na.mean[0]);
      const float sd = (c & 1) ? ((c & 2) ? na.stdv[3] : na.stdv[1]) : ((c & 2) ? na.stdv[2] : na.stdv[0]);
      t = (t - m) / sd;
    }
    out[i] = (T)t;   // i == (c * S + yy) * S + xx
  }
}

// batch entry: the job is the grid's second dimension and is read from the device table
__global__ __launch_bounds__(256) void batch_coeffs_kernel(const dgtd_preprocess_job* __restrict__ jobs, char* __restrict__ ws, int S) {
  const dgtd_preprocess_job jb = jobs[blockIdx.y];
  coeffs_body(jb, ws, S);
}
__global__ __launch_bounds__(256) void batch_resize_h_kernel(const dgtd_preprocess_job* __restrict__ jobs, const uint8_t* __restrict__ planes,
                                                             char* __restrict__ ws, int S) {
  const dgtd_preprocess_job jb = jobs[blockIdx.y];
  resize_h_body(jb, planes, ws, S);
}
template <typename T>
__global__ __launch_bounds__(256) void batch_resize_v_norm_kernel(const dgtd_preprocess_job* __restrict__ jobs, const char* __restrict__ ws,
                                                                  T* __restrict__ out_input, T* __restrict__ out_label, T* __restrict__ out_depth,
                                                                  int S, NormArgs na) {
  const dgtd_preprocess_job jb = jobs[blockIdx.y];
  resize_v_norm_body(jb, ws, out_input, out_label, out_depth, S, na);
}

// single-image entry: the one job is a kernel argument (64 bytes), so there is no table on the device and nothing to upload
__global__ __launch_bounds__(256) void one_coeffs_kernel(dgtd_preprocess_job jb, char* __restrict__ ws, int S) { coeffs_body(jb, ws, S); }
__global__ __launch_bounds__(256) void one_resize_h_kernel(dgtd_preprocess_job jb, const uint8_t* __restrict__ planes, char* __restrict__ ws, int S) {
  resize_h_body(jb, planes, ws, S);
}
template <typename T>
__global__ __launch_bounds__(256) void one_resize_v_norm_kernel(dgtd_preprocess_job jb, const char* __restrict__ ws, T* __restrict__ out, int S, NormArgs na) {
  resize_v_norm_body(jb, ws, out, (T*)nullptr, (T*)nullptr, S, na);
}

// a plane's sides are bounded so that every byte count below (H*W*C, H*S*C, the tables) stays far inside int64 and in + S inside int32
constexpr int MAX_SIDE = 1 << 24;
inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }
inline int64_t table_bytes(int in_size, int S) { return (int64_t)S * (2 + ksize_for(in_size, S)) * 4; }
// canonical workspace regions of one job, each rounded up to 16 bytes: mid, then tab_h, then tab_v
inline int64_t mid_bytes(int H, int C, int S) { return align16((int64_t)H * S * C); }
inline int64_t job_bytes(int H, int W, int C, int S) { return mid_bytes(H, C, S) + align16(table_bytes(W, S)) + align16(table_bytes(H, S)); }

// blocks in x of the three launches: 2S table threads; the largest H*C rows of S; S*S outputs of at most max_c channels
struct Grids { int coeffs, h, v; };
inline Grids grids_for(int64_t max_hc, int max_c, int S) {
  return {(int)cdiv(2 * (int64_t)S, 256), (int)std::min<int64_t>(cdiv(max_hc * S, 256), 1024),
          (int)std::min<int64_t>(cdiv((int64_t)S * S * max_c, 256), 1024)};
}

NormArgs norm_args(const float* mean_host, const float* std_host, int C) {
  NormArgs na;
  for (int c = 0; c < 4; ++c) { na.mean[c] = (mean_host && c < C) ? mean_host[c] : 0.f; na.stdv[c] = (std_host && c < C) ? std_host[c] : 1.f; }
  return na;
}

}  // namespace

extern "C" int64_t dgtd_preprocess_workspace(int Hin, int Win, int C, int S) {
  if (Hin < 1 || Win < 1 || S < 1 || C < 1 || C > 4) return -1;
  return job_bytes(Hin, Win, C, S);
}

extern "C" int dgtd_preprocess(const void* img_u8, void* out, const float* mean_host, const float* std_host, void* workspace, int Hin,
                               int Win, int C, int S, int flip, dgtd_dtype out_dt, dgtd_stream s) {
  DGTD_PROF(s, DGTD_HBM, (double)Hin * Win * C + (double)dgtd_esize(out_dt) * C * S * S, "dgtd_preprocess[%dx%dx%d->%d]", Hin, Win, C, S);
  DGTD_REQUIRE(Hin > 0 && Win > 0 && S > 0 && C >= 1 && C <= 4, "preprocess: bad sizes H=%d W=%d C=%d S=%d", Hin, Win, C, S);
  DGTD_REQUIRE((mean_host == nullptr) == (std_host == nullptr), "preprocess: mean and std go together");
  DGTD_REQUIRE(out_dt == DGTD_F32 || DGTD_IS_HALF(out_dt), "preprocess: bad output dtype %d", (int)out_dt);
  hipStream_t st = (hipStream_t)s;
  dgtd_preprocess_job jb = {};   // planes = img_u8, out_input = out: src_off, out_sel and batch are 0
  jb.tab_h_off = mid_bytes(Hin, C, S);
  jb.tab_v_off = jb.tab_h_off + align16(table_bytes(Win, S));
  jb.H = Hin; jb.W = Win; jb.C = C;
  jb.flip = flip;
  jb.normalize = mean_host != nullptr;
  const NormArgs na = norm_args(mean_host, std_host, C);
  const Grids g = grids_for((int64_t)Hin * C, C, S);
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(one_coeffs_kernel, dim3(g.coeffs), dim3(256), 0, st, jb, ws, S);
  DGTD_CHECK_LAUNCH("preprocess_coeffs");
  hipLaunchKernelGGL(one_resize_h_kernel, dim3(g.h), dim3(256), 0, st, jb, (const uint8_t*)img_u8, ws, S);
  DGTD_CHECK_LAUNCH("preprocess_horizontal");
  DGTD_DISPATCH(out_dt, hipLaunchKernelGGL(one_resize_v_norm_kernel<T_>, dim3(g.v), dim3(256), 0, st, jb, (const char*)ws, (T_*)out, S, na));
  DGTD_CHECK_LAUNCH("preprocess_vertical");
  return 0;
}

extern "C" int64_t dgtd_preprocess_batch_workspace(const dgtd_preprocess_job* jobs_host, int njobs, int S) {
  if (jobs_host == nullptr || njobs < 1 || S < 1) return -1;
  int64_t total = 0;
  for (int j = 0; j < njobs; ++j) {
    const dgtd_preprocess_job& jb = jobs_host[j];
    if (jb.H < 1 || jb.W < 1 || jb.H > MAX_SIDE || jb.W > MAX_SIDE || (jb.C != 1 && jb.C != 3)) return -1;
    total += job_bytes(jb.H, jb.W, jb.C, S);
  }
  return total;
}

extern "C" int dgtd_preprocess_batch(const void* planes_u8, int64_t planes_bytes, const dgtd_preprocess_job* jobs_dev,
                                     const dgtd_preprocess_job* jobs_host, int njobs, void* out_input, void* out_label, void* out_depth,
                                     int B, int S, const float* mean_host, const float* std_host, void* workspace,
                                     int64_t workspace_bytes, dgtd_dtype out_dt, dgtd_stream s) {
  // the job is the grid's second dimension (gridDim.y <= 65535)
  DGTD_REQUIRE(njobs >= 1 && njobs <= DGTD_PREPROCESS_BATCH_MAX_JOBS, "preprocess_batch: %d jobs, the grid's second dimension takes 1..%d", njobs,
               DGTD_PREPROCESS_BATCH_MAX_JOBS);
  DGTD_REQUIRE(jobs_dev != nullptr && jobs_host != nullptr && planes_u8 != nullptr && workspace != nullptr, "preprocess_batch: null buffer");
  DGTD_REQUIRE(B >= 1 && S >= 1 && (int64_t)S * S * 3 <= INT32_MAX, "preprocess_batch: bad sizes B=%d S=%d", B, S);
  DGTD_REQUIRE(planes_bytes >= 1 && workspace_bytes >= 1, "preprocess_batch: bad buffer sizes planes=%lld workspace=%lld", (long long)planes_bytes,
               (long long)workspace_bytes);
  DGTD_REQUIRE((mean_host == nullptr) == (std_host == nullptr), "preprocess_batch: mean and std go together");
  DGTD_REQUIRE(out_dt == DGTD_F32 || DGTD_IS_HALF(out_dt), "preprocess_batch: bad output dtype %d", (int)out_dt);
  DGTD_REQUIRE(((uintptr_t)planes_u8 & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)jobs_dev & 7) == 0,
               "preprocess_batch: planes and workspace must be 16-byte aligned, the job table 8-byte aligned");
  double bytes_in = 0.0;
  int64_t max_h = 0;
  for (int j = 0; j < njobs; ++j) {
    const dgtd_preprocess_job& jb = jobs_host[j];
    DGTD_REQUIRE(jb.H >= 1 && jb.W >= 1 && jb.H <= MAX_SIDE && jb.W <= MAX_SIDE && (jb.C == 1 || jb.C == 3),
                 "preprocess_batch: job %d: bad sizes H=%d W=%d C=%d (sides 1..%d, C 1 or 3)", j, jb.H, jb.W, jb.C, MAX_SIDE);
    DGTD_REQUIRE(jb.out_sel >= 0 && jb.out_sel <= 2 && jb.C == (jb.out_sel == 0 ? 3 : 1), "preprocess_batch: job %d: output %d does not take C=%d", j,
                 jb.out_sel, jb.C);
    DGTD_REQUIRE(jb.batch >= 0 && jb.batch < B, "preprocess_batch: job %d: batch index %d outside [0,%d)", j, jb.batch, B);
    DGTD_REQUIRE((jb.out_sel == 0 ? out_input : (jb.out_sel == 1 ? out_label : out_depth)) != nullptr, "preprocess_batch: job %d: output %d is null", j,
                 jb.out_sel);
    DGTD_REQUIRE(!jb.normalize || (jb.C == 3 && mean_host != nullptr), "preprocess_batch: job %d: Normalize needs C=3 and mean/std", j);
    const int64_t src = (int64_t)jb.H * jb.W * jb.C, mid = (int64_t)jb.H * S * jb.C;
    DGTD_REQUIRE(((jb.src_off | jb.mid_off | jb.tab_h_off | jb.tab_v_off) & 15) == 0, "preprocess_batch: job %d: offset not 16-byte aligned", j);
    DGTD_REQUIRE(jb.src_off >= 0 && jb.src_off <= planes_bytes - src, "preprocess_batch: job %d: plane [%lld,+%lld) outside the %lld bytes passed in", j,
                 (long long)jb.src_off, (long long)src, (long long)planes_bytes);
    DGTD_REQUIRE(jb.mid_off >= 0 && jb.mid_off <= workspace_bytes - mid && jb.tab_h_off >= 0 && jb.tab_h_off <= workspace_bytes - table_bytes(jb.W, S) &&
                     jb.tab_v_off >= 0 && jb.tab_v_off <= workspace_bytes - table_bytes(jb.H, S),
                 "preprocess_batch: job %d: workspace region outside the %lld bytes passed in", j, (long long)workspace_bytes);
    bytes_in += (double)src;
    max_h = std::max<int64_t>(max_h, (int64_t)jb.H * jb.C);
  }
  DGTD_PROF(s, DGTD_HBM, bytes_in + (double)dgtd_esize(out_dt) * 5.0 * B * S * S, "dgtd_preprocess_batch[%dx->%d]", njobs, S);
  hipStream_t st = (hipStream_t)s;
  const NormArgs na = norm_args(mean_host, std_host, 3);
  const Grids g = grids_for(max_h, 3, S);
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(batch_coeffs_kernel, dim3(g.coeffs, njobs), dim3(256), 0, st, jobs_dev, ws, S);
  DGTD_CHECK_LAUNCH("preprocess_batch_coeffs");
  hipLaunchKernelGGL(batch_resize_h_kernel, dim3(g.h, njobs), dim3(256), 0, st, jobs_dev, (const uint8_t*)planes_u8, ws, S);
  DGTD_CHECK_LAUNCH("preprocess_batch_horizontal");
  DGTD_DISPATCH(out_dt, hipLaunchKernelGGL(batch_resize_v_norm_kernel<T_>, dim3(g.v, njobs), dim3(256), 0, st, jobs_dev, (const char*)ws, (T_*)out_input,
                                           (T_*)out_label, (T_*)out_depth, S, na));
  DGTD_CHECK_LAUNCH("preprocess_batch_vertical");
  return 0;
}
