// Self-forcing distillation loss tails (reference: owl_wms/trainers/sf_vid_only.py:229-349) for gfx950.
//
// owlk_dmd_loss:    the DMD loss and its gradient to the rollout from the three no-grad velocities,
// owlk_critic_loss: the critic's masked flow-matching MSE and its gradient to the critic's output.
//
// Both read [B, N, F] tensors (F = C h w elements per frame, F % 8 == 0; bf16 as the cores emit and the
// loaders yield, or fp32, one flag for the video side and one for the velocities) in 8-element chunks, do all
// arithmetic in fp32 from the loaded values, keep per-workgroup partial sums and finish them in double
// in index order: no floating-point atomics, two calls on the same inputs give the same bits, and
// nothing is read back on the host.
//
// CausVid distillation tails (reference: owl_wms/trainers/causvid_vid_only.py:101-309), same rules:
// owlk_causvid_mix:      the per-frame noising of the teacher-forced rollout and of both losses,
// owlk_causvid_x0:       the one-step denoise of the mask's frames, the others copied,
// owlk_causvid_gen_loss: the DMD + regression losses and their gradient to the student's velocity.
#include "common.hpp"

namespace {

constexpr int kMaxSampleBlocks = 256;  // workgroups per sample (dmd) -- one wave reads them in <= 4 rounds
constexpr int kMaxBlocks = 2048;       // workgroups per launch (critic)

// 8 consecutive elements as fp32: bf16 (one 16-B load) or fp32 (two)
DEV void load8(const bf16* p, long chunk, float* f) { unpack8(((const bf16x8*)p)[chunk], f); }
DEV void load8(const float* p, long chunk, float* f) {
  const f32x4 a = ((const f32x4*)p)[2 * chunk], b = ((const f32x4*)p)[2 * chunk + 1];
#pragma unroll
  for (int e = 0; e < 4; ++e) f[e] = a[e], f[4 + e] = b[e];
}
DEV void store8(bf16* p, long chunk, const float* f) { ((bf16x8*)p)[chunk] = pack8(f); }
DEV void store8(float* p, long chunk, const float* f) {
  ((f32x4*)p)[2 * chunk] = f32x4{f[0], f[1], f[2], f[3]};
  ((f32x4*)p)[2 * chunk + 1] = f32x4{f[4], f[5], f[6], f[7]};
}

// the block's sum to partial[slot]: wave butterflies, then the four wave sums in order
DEV void block_partial(float acc, float* red4, float* partial, long slot) {
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[slot] = ((red4[0] + red4[1]) + red4[2]) + red4[3];
}

// the same double in every lane: lane l adds x[l], x[l + 64], ... in order, then a butterfly
DEV double wave_sum_f64(const float* __restrict__ x, int n) {
  double s = 0.0;
  for (int i = threadIdx.x & 63; i < n; i += 64) s += (double)x[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// true frames of mask[0 .. n), the same count in every lane (integers: exact in any order)
DEV long wave_count(const unsigned char* __restrict__ mask, long n) {
  int c = 0;
  for (long i = threadIdx.x & 63; i < n; i += 64) c += mask[i] != 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  return c;
}

// torch.nan_to_num(x, nan=0.0) in fp32
DEV float nan_to_num(float x) {
  if (x != x) return 0.f;
  return fminf(fmaxf(x, -3.402823466e+38f), 3.402823466e+38f);
}

// guided teacher velocity of 8 elements (null v_uncond: the conditional one) and the critic's
template <typename V>
DEV void teacher8(const V* vc, const V* vu, long chunk, float cfg, float* vt) {
  load8(vc, chunk, vt);
  if (vu) {
    float u[8];
    load8(vu, chunk, u);
#pragma unroll
    for (int e = 0; e < 8; ++e) vt[e] = u[e] + cfg * (vt[e] - u[e]);
  }
}

// ---- pass 1: absum[b * gridDim.x + block] = sum over the block's share of sample b of
//      |video - noisy + ts v_t|  (video - mu_teacher, sf_vid_only.py:318-323)
template <typename T, typename V>
__global__ __launch_bounds__(256) void dmd_absum_k(const T* __restrict__ video, const T* __restrict__ noisy,
                                                   const V* __restrict__ vc, const V* __restrict__ vu,
                                                   const float* __restrict__ ts, long N, long F8, float cfg,
                                                   float* __restrict__ absum) {
  __shared__ float red[4];
  const long b = blockIdx.y, per = N * F8;
  float acc = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
    const long chunk = b * per + i;
    const float t = ts[b * N + i / F8];
    float x[8], y[8], vt[8];
    load8(video, chunk, x);
    load8(noisy, chunk, y);
    teacher8(vc, vu, chunk, cfg, vt);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc += fabsf((x[e] - y[e]) + t * vt[e]);
  }
  block_partial(acc, red, absum, b * gridDim.x + blockIdx.x);
}

// ---- pass 2: g = nan_to_num(ts (v_t - v_k) / norm_b), norm_b the sample's mean of pass 1;
//      dvideo = g / M on the mask's frames and 0 elsewhere, sq[b * gridDim.x + block] = sum g^2 there
template <typename T, typename V>
__global__ __launch_bounds__(256) void dmd_grad_k(const V* __restrict__ vc, const V* __restrict__ vu,
                                                  const V* __restrict__ vk, const float* __restrict__ ts,
                                                  const unsigned char* __restrict__ mask, long B, long N, long F8,
                                                  float cfg, const float* __restrict__ absum, T* __restrict__ dvideo,
                                                  float* __restrict__ sq) {
  __shared__ float red[4];
  const long b = blockIdx.y, per = N * F8;
  const float norm = (float)(wave_sum_f64(absum + b * gridDim.x, gridDim.x) / (double)(per * 8));
  const float inv_m = (float)(1.0 / (double)(wave_count(mask, B * N) * F8 * 8));  // inf at M = 0: unused then
  float acc = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
    const long chunk = b * per + i, frame = b * N + i / F8;
    float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (mask[frame]) {
      const float t = ts[frame];
      float vt[8], k[8];
      teacher8(vc, vu, chunk, cfg, vt);
      load8(vk, chunk, k);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float ge = nan_to_num((t * (vt[e] - k[e])) / norm);
        acc += ge * ge;
        g[e] = ge * inv_m;
      }
    }
    store8(dvideo, chunk, g);
  }
  block_partial(acc, red, sq, b * gridDim.x + blockIdx.x);
}

// loss = scale * (the partials' sum in double, in index order) / denom; denom < 0: the mask's true
// frames times F, counted here (0 of them: 0 / 0 = NaN, the mean over nothing)
__global__ __launch_bounds__(64) void loss_finish_k(const float* __restrict__ partial, int n, double scale,
                                                    long denom, const unsigned char* __restrict__ mask, long frames,
                                                    long F, float* __restrict__ loss) {
  const double s = wave_sum_f64(partial, n);
  const long m = denom < 0 ? wave_count(mask, frames) * F : denom;
  if (threadIdx.x == 0) loss[0] = (float)(scale * s / (double)m);
}

// ---- critic: d = m (pred - (z - video)); dpred = gscale d in pred's type; partial[block] = sum d^2
template <typename T, typename V>
__global__ __launch_bounds__(256) void critic_k(const V* __restrict__ pred, const T* __restrict__ z,
                                                const T* __restrict__ video, const unsigned char* __restrict__ mask,
                                                long n8, long F8, float gscale, V* __restrict__ dpred,
                                                float* __restrict__ partial) {
  __shared__ float red[4];
  float acc = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (mask[i / F8]) {
      float p[8], zz[8], x[8];
      load8(pred, i, p);
      load8(z, i, zz);
      load8(video, i, x);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = p[e] - (zz[e] - x[e]);
        acc += d * d;
        g[e] = gscale * d;
      }
    }
    store8(dpred, i, g);
  }
  block_partial(acc, red, partial, blockIdx.x);
}

// ---- CausVid ---------------------------------------------------------------------------------------
// 8 consecutive elements moved as they are (no conversion: NaN payloads and signed zeros survive)
DEV void copy8(const bf16* src, bf16* dst, long chunk) { ((bf16x8*)dst)[chunk] = ((const bf16x8*)src)[chunk]; }
DEV void copy8(const float* src, float* dst, long chunk) {
  ((f32x4*)dst)[2 * chunk] = ((const f32x4*)src)[2 * chunk];
  ((f32x4*)dst)[2 * chunk + 1] = ((const f32x4*)src)[2 * chunk + 1];
}

// noisy = x (1 - t) + z t, t = ts[frame] on the mask's frames (all of them without a mask) and noise_prev
// elsewhere; the thread with a frame's first chunk writes ts_full[frame] = t
template <typename T>
__global__ __launch_bounds__(256) void causvid_mix_k(const T* __restrict__ x, const T* __restrict__ z,
                                                     const float* __restrict__ ts,
                                                     const unsigned char* __restrict__ mask, float noise_prev,
                                                     long n8, long F8, T* __restrict__ noisy,
                                                     float* __restrict__ ts_full) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    const long frame = i / F8;
    const float t = (!mask || mask[frame]) ? ts[frame] : noise_prev;
    float a[8], b[8];
    load8(x, i, a);
    load8(z, i, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = a[e] * (1.f - t) + b[e] * t;
    store8(noisy, i, a);
    if (ts_full && i == frame * F8) ts_full[frame] = t;
  }
}

// out = noisy - ts_full v on the mask's frames, clean (bit for bit) elsewhere
template <typename T, typename V>
__global__ __launch_bounds__(256) void causvid_x0_k(const T* __restrict__ noisy, const T* __restrict__ clean,
                                                    const V* __restrict__ v, const float* __restrict__ ts_full,
                                                    const unsigned char* __restrict__ mask, long n8, long F8,
                                                    T* __restrict__ out) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    const long frame = i / F8;
    if (!mask[frame]) {
      copy8(clean, out, i);
      continue;
    }
    const float t = ts_full[frame];
    float a[8], b[8];
    load8(noisy, i, a);
    load8(v, i, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = a[e] - t * b[e];
    store8(out, i, a);
  }
}

// ---- generator loss, pass 2 (pass 1 is dmd_absum_k on out, noisy2, ts2): on the mask's frames
//      g = nan_to_num(ts2 (v_t - v_k) / norm_b), r = out - orig, dv = -ts_full (g + 2 w r) / n in the
//      velocities' type, exact zeros elsewhere; sqg / sqr[b * gridDim.x + block] = sum g^2 / sum r^2
template <typename T, typename V>
__global__ __launch_bounds__(256) void causvid_gen_k(const T* __restrict__ out, const T* __restrict__ orig,
                                                     const V* __restrict__ vc, const V* __restrict__ vu,
                                                     const V* __restrict__ vk, const float* __restrict__ ts2,
                                                     const float* __restrict__ ts_full,
                                                     const unsigned char* __restrict__ mask, long N, long F8,
                                                     float cfg, float w2, float inv_n,
                                                     const float* __restrict__ absum, V* __restrict__ dv,
                                                     float* __restrict__ sqg, float* __restrict__ sqr) {
  __shared__ float red_g[4], red_r[4];
  const long b = blockIdx.y, per = N * F8;
  const float norm = (float)(wave_sum_f64(absum + b * gridDim.x, gridDim.x) / (double)(per * 8));
  float acc_g = 0.f, acc_r = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
    const long chunk = b * per + i, frame = b * N + i / F8;
    float d[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (mask[frame]) {
      const float t2 = ts2[frame], tf = ts_full[frame];
      float vt[8], k[8], o[8], x[8];
      teacher8(vc, vu, chunk, cfg, vt);
      load8(vk, chunk, k);
      load8(out, chunk, o);
      load8(orig, chunk, x);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float g = nan_to_num((t2 * (vt[e] - k[e])) / norm), r = o[e] - x[e];
        acc_g += g * g;
        acc_r += r * r;
        d[e] = -(tf * (g + w2 * r)) * inv_n;
      }
    }
    store8(dv, chunk, d);
  }
  block_partial(acc_g, red_g, sqg, b * gridDim.x + blockIdx.x);
  block_partial(acc_r, red_r, sqr, b * gridDim.x + blockIdx.x);
}

// losses = {0.5 sum g^2 / n, sum r^2 / n}, the partials summed in double in index order
__global__ __launch_bounds__(64) void causvid_gen_finish_k(const float* __restrict__ sqg,
                                                           const float* __restrict__ sqr, int np, long n,
                                                           float* __restrict__ losses) {
  const double g = wave_sum_f64(sqg, np), r = wave_sum_f64(sqr, np);
  if (threadIdx.x == 0) {
    losses[0] = (float)(0.5 * g / (double)n);
    losses[1] = (float)(r / (double)n);
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// workgroups per sample: two chunks per thread, at most kMaxSampleBlocks, about 2048 per launch
inline int dmd_sample_blocks(long B, long N, long F) {
  long nb = (N * (F / 8) + 511) / 512, cap = kMaxBlocks / B;
  if (cap > kMaxSampleBlocks) cap = kMaxSampleBlocks;
  if (nb > cap) nb = cap;
  return nb < 1 ? 1 : (int)nb;
}

inline int critic_blocks(long n) {
  const long nb = (n / 8 + 255) / 256;
  return nb > kMaxBlocks ? kMaxBlocks : (nb < 1 ? 1 : (int)nb);
}

template <typename T, typename V>
void launch_dmd(dim3 grid, hipStream_t s, const void* video, const void* noisy, const void* vc, const void* vu,
                const void* vk, const float* ts, const unsigned char* m, long B, long N, long F8, float cfg,
                float* absum, void* dvideo, float* sq) {
  hipLaunchKernelGGL((dmd_absum_k<T, V>), grid, dim3(256), 0, s, (const T*)video, (const T*)noisy, (const V*)vc,
                     (const V*)vu, ts, N, F8, cfg, absum);
  hipLaunchKernelGGL((dmd_grad_k<T, V>), grid, dim3(256), 0, s, (const V*)vc, (const V*)vu, (const V*)vk, ts, m, B,
                     N, F8, cfg, absum, (T*)dvideo, sq);
}

template <typename T, typename V>
void launch_critic(int nb, hipStream_t s, const void* pred, const void* z, const void* video,
                   const unsigned char* m, long n8, long F8, float gscale, void* dpred, float* partial) {
  hipLaunchKernelGGL((critic_k<T, V>), dim3(nb), dim3(256), 0, s, (const V*)pred, (const T*)z, (const T*)video, m,
                     n8, F8, gscale, (V*)dpred, partial);
}

template <typename T>
void launch_mix(int nb, hipStream_t s, const void* x, const void* z, const float* ts, const unsigned char* m,
                float noise_prev, long n8, long F8, void* noisy, float* ts_full) {
  hipLaunchKernelGGL((causvid_mix_k<T>), dim3(nb), dim3(256), 0, s, (const T*)x, (const T*)z, ts, m, noise_prev, n8,
                     F8, (T*)noisy, ts_full);
}

template <typename T, typename V>
void launch_x0(int nb, hipStream_t s, const void* noisy, const void* clean, const void* v, const float* ts_full,
               const unsigned char* m, long n8, long F8, void* out) {
  hipLaunchKernelGGL((causvid_x0_k<T, V>), dim3(nb), dim3(256), 0, s, (const T*)noisy, (const T*)clean,
                     (const V*)v, ts_full, m, n8, F8, (T*)out);
}

template <typename T, typename V>
void launch_gen(dim3 grid, hipStream_t s, const void* out, const void* orig, const void* noisy2, const void* vc,
                const void* vu, const void* vk, const float* ts2, const float* ts_full, const unsigned char* m,
                long N, long F8, float cfg, float w2, float inv_n, float* absum, void* dv, float* sqg,
                float* sqr) {
  hipLaunchKernelGGL((dmd_absum_k<T, V>), grid, dim3(256), 0, s, (const T*)out, (const T*)noisy2, (const V*)vc,
                     (const V*)vu, ts2, N, F8, cfg, absum);
  hipLaunchKernelGGL((causvid_gen_k<T, V>), grid, dim3(256), 0, s, (const T*)out, (const T*)orig, (const V*)vc,
                     (const V*)vu, (const V*)vk, ts2, ts_full, m, N, F8, cfg, w2, inv_n, absum, (V*)dv, sqg, sqr);
}

}  // namespace

extern "C" long owlk_dmd_loss_ws_bytes(long B, long N, long F) {
  if (B <= 0 || N <= 0 || F <= 0 || F % 8 != 0 || B > 65535) return 0;
  return 2 * B * dmd_sample_blocks(B, N, F) * (long)sizeof(float);
}

extern "C" int owlk_dmd_loss(const void* video, const void* noisy, int in_f32, const void* v_cond,
                             const void* v_uncond, const void* v_critic, int v_f32, const float* ts,
                             const void* mask, long B, long N, long F, float cfg_scale, float* loss, void* dvideo,
                             void* ws, long ws_bytes, void* stream) {
  OWLK_REQUIRE(B > 0 && N > 0 && F > 0 && B <= 65535, "dmd_loss: bad sizes B=%ld N=%ld F=%ld", B, N, F);
  OWLK_REQUIRE(F % 8 == 0, "dmd_loss: F=%ld elements per frame must be a multiple of 8", F);
  OWLK_REQUIRE(video && noisy && v_cond && v_critic && ts && mask && loss && dvideo,
               "dmd_loss: video, noisy, v_cond, v_critic, ts, mask, loss and dvideo are required");
  OWLK_REQUIRE(aligned16(video) && aligned16(noisy) && aligned16(v_cond) && aligned16(v_uncond) &&
                   aligned16(v_critic) && aligned16(dvideo),
               "dmd_loss: tensors must be 16-byte aligned");
  const int nb = dmd_sample_blocks(B, N, F);
  OWLK_REQUIRE(ws && ws_bytes >= 2 * B * nb * (long)sizeof(float) && ((uintptr_t)ws & 3) == 0,
               "dmd_loss: workspace of %ld bytes, owlk_dmd_loss_ws_bytes asks for %ld", ws_bytes,
               2 * B * nb * (long)sizeof(float));
  float* absum = (float*)ws;
  float* sq = absum + B * nb;
  const dim3 grid((unsigned)nb, (unsigned)B);
  const unsigned char* m = (const unsigned char*)mask;
  hipStream_t s = (hipStream_t)stream;
  auto go = in_f32 ? (v_f32 ? launch_dmd<float, float> : launch_dmd<float, bf16>)
                   : (v_f32 ? launch_dmd<bf16, float> : launch_dmd<bf16, bf16>);
  go(grid, s, video, noisy, v_cond, v_uncond, v_critic, ts, m, B, N, F / 8, cfg_scale, absum, dvideo, sq);
  if (int rc = owlk::check_launch("dmd_loss")) return rc;
  hipLaunchKernelGGL(loss_finish_k, dim3(1), dim3(64), 0, s, sq, (int)(B * nb), 0.5, -1L, m, B * N, F, loss);
  return owlk::check_launch("dmd_loss");
}

extern "C" long owlk_critic_loss_ws_bytes(long n) {
  if (n <= 0 || n % 8 != 0) return 0;
  return critic_blocks(n) * (long)sizeof(float);
}

extern "C" int owlk_critic_loss(const void* pred, int pred_f32, const void* z, const void* video, int in_f32,
                                const void* mask, long B, long N, long F, float gscale, float* loss, void* dpred,
                                void* ws, long ws_bytes, void* stream) {
  OWLK_REQUIRE(B > 0 && N > 0 && F > 0, "critic_loss: bad sizes B=%ld N=%ld F=%ld", B, N, F);
  OWLK_REQUIRE(F % 8 == 0, "critic_loss: F=%ld elements per frame must be a multiple of 8", F);
  OWLK_REQUIRE(pred && z && video && mask && loss && dpred,
               "critic_loss: pred, z, video, mask, loss and dpred are required");
  OWLK_REQUIRE(aligned16(pred) && aligned16(z) && aligned16(video) && aligned16(dpred),
               "critic_loss: tensors must be 16-byte aligned");
  const long n = B * N * F;
  const int nb = critic_blocks(n);
  OWLK_REQUIRE(ws && ws_bytes >= nb * (long)sizeof(float) && ((uintptr_t)ws & 3) == 0,
               "critic_loss: workspace of %ld bytes, owlk_critic_loss_ws_bytes asks for %ld", ws_bytes,
               nb * (long)sizeof(float));
  float* partial = (float*)ws;
  const unsigned char* m = (const unsigned char*)mask;
  hipStream_t s = (hipStream_t)stream;
  auto go = in_f32 ? (pred_f32 ? launch_critic<float, float> : launch_critic<float, bf16>)
                   : (pred_f32 ? launch_critic<bf16, float> : launch_critic<bf16, bf16>);
  go(nb, s, pred, z, video, m, n / 8, F / 8, gscale, dpred, partial);
  if (int rc = owlk::check_launch("critic_loss")) return rc;
  hipLaunchKernelGGL(loss_finish_k, dim3(1), dim3(64), 0, s, partial, nb, 1.0, n, m, 0L, F, loss);
  return owlk::check_launch("critic_loss");
}

extern "C" int owlk_causvid_mix(const void* x, const void* z, int in_f32, const float* ts, const void* mask,
                                float noise_prev, long B, long N, long F, void* noisy, float* ts_full,
                                void* stream) {
  OWLK_REQUIRE(B > 0 && N > 0 && F > 0, "causvid_mix: bad sizes B=%ld N=%ld F=%ld", B, N, F);
  OWLK_REQUIRE(F % 8 == 0, "causvid_mix: F=%ld elements per frame must be a multiple of 8", F);
  OWLK_REQUIRE(x && z && ts && noisy, "causvid_mix: x, z, ts and noisy are required");
  OWLK_REQUIRE(aligned16(x) && aligned16(z) && aligned16(noisy), "causvid_mix: tensors must be 16-byte aligned");
  OWLK_REQUIRE(((uintptr_t)ts & 3) == 0 && ((uintptr_t)ts_full & 3) == 0,
               "causvid_mix: ts and ts_full must be 4-byte aligned");
  const long n = B * N * F;
  auto go = in_f32 ? launch_mix<float> : launch_mix<bf16>;
  go(critic_blocks(n), (hipStream_t)stream, x, z, ts, (const unsigned char*)mask, noise_prev, n / 8, F / 8, noisy,
     ts_full);
  return owlk::check_launch("causvid_mix");
}

extern "C" int owlk_causvid_x0(const void* noisy, const void* clean, int in_f32, const void* v, int v_f32,
                               const float* ts_full, const void* mask, long B, long N, long F, void* out,
                               void* stream) {
  OWLK_REQUIRE(B > 0 && N > 0 && F > 0, "causvid_x0: bad sizes B=%ld N=%ld F=%ld", B, N, F);
  OWLK_REQUIRE(F % 8 == 0, "causvid_x0: F=%ld elements per frame must be a multiple of 8", F);
  OWLK_REQUIRE(noisy && clean && v && ts_full && mask && out,
               "causvid_x0: noisy, clean, v, ts_full, mask and out are required");
  OWLK_REQUIRE(aligned16(noisy) && aligned16(clean) && aligned16(v) && aligned16(out),
               "causvid_x0: tensors must be 16-byte aligned");
  OWLK_REQUIRE(((uintptr_t)ts_full & 3) == 0, "causvid_x0: ts_full must be 4-byte aligned");
  const long n = B * N * F;
  auto go = in_f32 ? (v_f32 ? launch_x0<float, float> : launch_x0<float, bf16>)
                   : (v_f32 ? launch_x0<bf16, float> : launch_x0<bf16, bf16>);
  go(critic_blocks(n), (hipStream_t)stream, noisy, clean, v, ts_full, (const unsigned char*)mask, n / 8, F / 8, out);
  return owlk::check_launch("causvid_x0");
}

extern "C" long owlk_causvid_gen_loss_ws_bytes(long B, long N, long F) {
  if (B <= 0 || N <= 0 || F <= 0 || F % 8 != 0 || B > 65535) return 0;
  return 3 * B * dmd_sample_blocks(B, N, F) * (long)sizeof(float);
}

extern "C" int owlk_causvid_gen_loss(const void* out, const void* orig, const void* noisy2, int in_f32,
                                     const void* v_cond, const void* v_uncond, const void* v_critic, int v_f32,
                                     const float* ts2, const float* ts_full, const void* mask, long B, long N,
                                     long F, float cfg_scale, float reg_weight, float* losses, void* dv, void* ws,
                                     long ws_bytes, void* stream) {
  OWLK_REQUIRE(B > 0 && N > 0 && F > 0 && B <= 65535, "causvid_gen_loss: bad sizes B=%ld N=%ld F=%ld", B, N, F);
  OWLK_REQUIRE(F % 8 == 0, "causvid_gen_loss: F=%ld elements per frame must be a multiple of 8", F);
  OWLK_REQUIRE(out && orig && noisy2 && v_cond && v_critic && ts2 && ts_full && mask && losses && dv,
               "causvid_gen_loss: out, orig, noisy2, v_cond, v_critic, ts2, ts_full, mask, losses and dv are "
               "required");
  OWLK_REQUIRE(aligned16(out) && aligned16(orig) && aligned16(noisy2) && aligned16(v_cond) &&
                   aligned16(v_uncond) && aligned16(v_critic) && aligned16(dv),
               "causvid_gen_loss: tensors must be 16-byte aligned");
  OWLK_REQUIRE((((uintptr_t)ts2 | (uintptr_t)ts_full | (uintptr_t)losses) & 3) == 0,
               "causvid_gen_loss: ts2, ts_full and losses must be 4-byte aligned");
  const int nb = dmd_sample_blocks(B, N, F);
  OWLK_REQUIRE(ws && ws_bytes >= 3 * B * nb * (long)sizeof(float) && ((uintptr_t)ws & 3) == 0,
               "causvid_gen_loss: workspace of %ld bytes, owlk_causvid_gen_loss_ws_bytes asks for %ld", ws_bytes,
               3 * B * nb * (long)sizeof(float));
  float* absum = (float*)ws;
  float* sqg = absum + B * nb;
  float* sqr = sqg + B * nb;
  const dim3 grid((unsigned)nb, (unsigned)B);
  const long n = B * N * F;
  hipStream_t s = (hipStream_t)stream;
  auto go = in_f32 ? (v_f32 ? launch_gen<float, float> : launch_gen<float, bf16>)
                   : (v_f32 ? launch_gen<bf16, float> : launch_gen<bf16, bf16>);
  go(grid, s, out, orig, noisy2, v_cond, v_uncond, v_critic, ts2, ts_full, (const unsigned char*)mask, N, F / 8,
     cfg_scale, 2.f * reg_weight, (float)(1.0 / (double)n), absum, dv, sqg, sqr);
  if (int rc = owlk::check_launch("causvid_gen_loss")) return rc;
  hipLaunchKernelGGL(causvid_gen_finish_k, dim3(1), dim3(64), 0, s, sqg, sqr, (int)(B * nb), n, losses);
  return owlk::check_launch("causvid_gen_loss");
}
