// Gradient guard for gfx950: the global L2 norm of a list of fp32 gradient buffers (the reducer's flat
// buckets, utils/grad_reducer.py), whether it is finite, and the fused norm clip.
//
// What it stands in for: the reference's distillation step unscales, clips and lets GradScaler.step skip
// the optimizer step on an inf / NaN gradient (sf_vid_only.py:503-508); the RFT trainers clip
// (rft_trainer.py:197-199).  Here the gradients are fp32 and nothing is scaled, so one reduction gives
// the clip coefficient and the skip decision both.
//
//   pass 1  guard_sumsq_k   one workgroup per kChunk consecutive elements of one buffer: fp32 sum of squares
//                     (16-B loads, a scalar tail on a buffer's last chunk), wave butterflies, the four wave
//                     sums in order, one partial per workgroup in the workspace
//   pass 2  guard_finish_k  one wave adds the partials in double, lane l taking l, l + 64, ... in order, then a
//                     butterfly: state = {norm, clip_coef, finite, 0}
//   pass 3  guard_scale_k   (max_norm > 0 only) every thread reads state and returns when clip_coef >= 1 or the
//                     sum is not finite, before touching a gradient; otherwise g *= clip_coef
//
// The split depends on (count, n[]) alone: buffer i owns ceil(n[i] / kChunk) workgroups, in buffer order.
// Nothing reads the CU count or the CU reserve, there are no atomics and no workgroup waits for another,
// so two calls give the same bits on every box.  A NaN or an Inf element makes its partial non-finite, and
// so does a partial that overflows fp32: finite = 0, and the step is skipped by the caller.
#include "common.hpp"

#include <cmath>

namespace {

constexpr int kMaxG = 16;          // buffers per launch (OWLK_GRAD_GUARD_TABLE)
constexpr long kChunk = 1L << 16;  // elements per workgroup: 64 16-B loads per thread
constexpr long kMaxBlocks = 1L << 22;

struct GuardPtrs {
  float* g[kMaxG];
  long n[kMaxG];
  unsigned first[kMaxG + 1];  // first[i]: the launch's first workgroup of buffer i; first[k]: their count
};

// the workgroup's buffer: -> its share's first element, and how many elements the buffer has from there on
// (the share is the first kChunk of them, or all when fewer)
DEV float* my_chunk(const GuardPtrs& P, long& rest) {
  int z = 0;
  while (blockIdx.x >= P.first[z + 1]) ++z;  // uniform: at most kMaxG - 1 scalar steps
  const long start = (long)(blockIdx.x - P.first[z]) * kChunk;
  rest = P.n[z] - start;
  return P.g[z] + start;
}

DEV float sq4(const f32x4 v, float acc) { return acc + ((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3])); }

__global__ __launch_bounds__(256) void guard_sumsq_k(GuardPtrs P, float* __restrict__ partial) {
  __shared__ float red[4];
  long rest;
  const float* __restrict__ g = my_chunk(P, rest);
  const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  // `rest` itself is branched on: with len = min(rest, kChunk) taken first and compared with kChunk, hipcc
  // (ROCm 7) selected the short chunk's length on a stale SCC and read a whole chunk from a short buffer
  if (rest >= kChunk) {  // a whole chunk: no bounds to check
#pragma unroll 2
    for (int i = 0; i < (int)(kChunk / 4); i += 4 * 256) {
      const f32x4 v0 = g4[i + threadIdx.x], v1 = g4[i + 256 + threadIdx.x], v2 = g4[i + 512 + threadIdx.x],
                  v3 = g4[i + 768 + threadIdx.x];
      a0 = sq4(v0, a0);
      a1 = sq4(v1, a1);
      a2 = sq4(v2, a2);
      a3 = sq4(v3, a3);
    }
  } else {  // the buffer's last chunk: rest < kChunk elements, the last rest % 4 of them one by one
    const int len = (int)rest, n4 = len >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) a0 = sq4(g4[i], a0);
    const int t = (n4 << 2) + threadIdx.x;
    if (t < len) a1 = g[t] * g[t];
  }
  float acc = (a0 + a1) + (a2 + a3);
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(64) void guard_finish_k(const float* __restrict__ partial, int n, float max_norm,
                                               float* __restrict__ state) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 64) s += (double)partial[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x != 0) return;
  const bool finite = s - s == 0.0;  // false for NaN and +-Inf
  const float norm = (float)sqrt(s);
  float coef = 1.f;
  if (finite && max_norm > 0.f) coef = fminf(1.f, __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f)));
  *reinterpret_cast<f32x4*>(state) = f32x4{norm, coef, finite ? 1.f : 0.f, 0.f};
}

__global__ __launch_bounds__(256) void guard_scale_k(GuardPtrs P, const float* __restrict__ state) {
  const float coef = state[1];
  if (!(coef < 1.f) || state[2] == 0.f) return;  // nothing to clip, or a skipped step: no traffic
  long rest;
  float* g = my_chunk(P, rest);
  int len = (int)kChunk;
  if (rest < kChunk) len = (int)rest;
  f32x4* g4 = reinterpret_cast<f32x4*>(g);
  const int n4 = len >> 2;
#pragma unroll 4
  for (int i = threadIdx.x; i < n4; i += 256) {
    f32x4 v = g4[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] *= coef;
    g4[i] = v;
  }
  const int t = (n4 << 2) + threadIdx.x;
  if (t < len) g[t] *= coef;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline long chunks(long n) { return (n + kChunk - 1) / kChunk; }

// total workgroups over the buffers, or -1 on a bad argument
long total_blocks(int count, const long* n) {
  if (count < 0 || (count > 0 && !n)) return -1;
  long b = 0;
  for (int i = 0; i < count; ++i) {
    if (n[i] < 0) return -1;
    b += chunks(n[i]);
    if (b > kMaxBlocks) return -1;
  }
  return b;
}

// the pointer table of buffers [base, base + k); -> its workgroups
unsigned fill(GuardPtrs& P, float* const* g, const long* n, int base, int k) {
  unsigned b = 0;
  for (int i = 0; i < k; ++i) {
    P.g[i] = g[base + i];
    P.n[i] = n[base + i];
    P.first[i] = b;
    b += (unsigned)chunks(n[base + i]);
  }
  for (int i = k; i <= kMaxG; ++i) P.first[i] = b;
  return b;
}

}  // namespace

extern "C" long owlk_grad_guard_ws_bytes(int count, const long* n) {
  const long b = total_blocks(count, n);
  return b < 0 ? 0 : b * (long)sizeof(float);
}

extern "C" int owlk_grad_guard(int count, float* const* g, const long* n, float max_norm, float* state, void* ws,
                               long ws_bytes, void* stream) {
  OWLK_REQUIRE(count >= 0 && state && (count == 0 || (g && n)), "grad_guard: count >= 0, g, n and state are required");
  OWLK_REQUIRE(aligned16(state), "grad_guard: state must be 16-byte aligned");
  for (int i = 0; i < count; ++i) {
    OWLK_REQUIRE(n[i] >= 0, "grad_guard: buffer %d has negative length %ld", i, n[i]);
    OWLK_REQUIRE(g[i] || n[i] == 0, "grad_guard: buffer %d is a null pointer", i);
    OWLK_REQUIRE(aligned16(g[i]), "grad_guard: buffer %d must be 16-byte aligned", i);
  }
  const long blocks = total_blocks(count, n);
  OWLK_REQUIRE(blocks >= 0, "grad_guard: more than %ld workgroups of %ld elements", kMaxBlocks, kChunk);
  const long need = blocks * (long)sizeof(float);
  OWLK_REQUIRE(ws_bytes >= need && (need == 0 || (ws && ((uintptr_t)ws & 3) == 0)),
               "grad_guard: workspace of %ld bytes (4-byte aligned), owlk_grad_guard_ws_bytes asks for %ld", ws_bytes,
               need);
  hipStream_t s = (hipStream_t)stream;
  float* partial = (float*)ws;
  long slot = 0;
  for (int base = 0; base < count; base += kMaxG) {
    GuardPtrs P{};
    const unsigned b = fill(P, g, n, base, count - base < kMaxG ? count - base : kMaxG);
    if (b) hipLaunchKernelGGL(guard_sumsq_k, dim3(b), dim3(256), 0, s, P, partial + slot);
    slot += b;
  }
  hipLaunchKernelGGL(guard_finish_k, dim3(1), dim3(64), 0, s, partial, (int)blocks, max_norm, state);
  if (int rc = owlk::check_launch("grad_guard")) return rc;
  if (!(max_norm > 0.f)) return 0;
  for (int base = 0; base < count; base += kMaxG) {
    GuardPtrs P{};
    const unsigned b = fill(P, g, n, base, count - base < kMaxG ? count - base : kMaxG);
    if (b) hipLaunchKernelGGL(guard_scale_k, dim3(b), dim3(256), 0, s, P, state);
  }
  return owlk::check_launch("grad_guard");
}
