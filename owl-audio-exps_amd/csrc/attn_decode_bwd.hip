// Backward of the unmasked KV-cache decode attention (gfx950, head_dim 64 and 128).
//
// The gradient autograd forms for the cache branch of the reference's attention (attn.py:86-107)
// when a self-forcing rollout backpropagates through one decode step (sf_vid_only.py:181-188):
// Lq queries of the new frame(s) against Lkv keys = [cache | the Lnew new rows], no mask, the cache
// a constant.  With P recomputed from the forward's base-2 log-sum-exp,
//   P = exp2(scale log2e Q K^T - lse),  dP = dO V^T,  dS = P o (dP - delta),
//   dQ = scale dS K            over all Lkv keys,
//   dK = scale dS^T Q, dV = P^T dO   for the last Lnew key rows only.
//
// A decode step has only B x H chains, so the keys are split over workgroups: grid = (splits, H, B),
// one split = KS keys (a function of head_dim only, so the split count depends on the shapes alone and
// the gradients are bitwise the same on every device and from run to run).
//   phase 1 (every split): the split's K and V rows are staged once in LDS; wave w owns the 16-query
//     tiles w, w + 4, ... with the query on the lane column (Q / dO rows as B operands in registers, as
//     attn_fwd16_split_k): S^T = K Q^T and dP^T = V dO^T per 32 keys, dS^T from the accumulators as the
//     B operand of dQ^T += K^T dS^T (K^T through ds_read_b64_tr_b16).  The wave stores its fp32 partial
//     dQ rows of this split to the workspace [B, H, split, Lq, D].
//   phase 2 (the splits that hold new keys): the key on the lane column (K / V rows as B operands in
//     registers, as attn_bwd_dkdv16_k), 64-query tiles of Q and dO staged in LDS over the K/V image;
//     dV^T += dO^T P and dK^T += Q^T dS stay in registers and are stored directly: a key belongs to
//     one split, so nothing is summed across workgroups.
// attn_decode_bwd_reduce_k then adds the partials in split order and writes bf16 dQ.  No float
// atomics, no flags, nothing waits on another workgroup.
#include "attn_common.hpp"

namespace {

constexpr float LOG2E = 1.4426950408889634f;

template <int D>
struct DecBwdCfg {
  static constexpr int KS = D == 64 ? 256 : 128;  // keys per split: a 64 KiB K | V image either way
  static constexpr int NSUB = D / 64;             // 64-column sub-tiles (128-B rows)
  static constexpr int NKD = D / 32;              // k steps over d
  static constexpr int NDS = D / 16;              // 16-column d tiles of the transposed outputs
  static constexpr int SUBK = KS * 128;           // bytes of one K / V sub-tile
  static constexpr int SUBQ = 64 * 128;           // bytes of one Q / dO sub-tile (phase 2)
  static constexpr int NKT = D == 64 ? 2 : 1;     // 16-key tiles per wave and pass (phase 2)
  static constexpr int KVB = 2 * NSUB * SUBK;
  static constexpr int QDB = 2 * NSUB * SUBQ + 2 * 64 * 4;  // Q | dO | lse | delta
  static constexpr int SMEM = KVB > QDB ? KVB : QDB;
};

static int splits_of(long Lkv, int head_dim) {
  const long ks = head_dim == 64 ? DecBwdCfg<64>::KS : DecBwdCfg<128>::KS;
  return (int)((Lkv + ks - 1) / ks);
}

struct DecBwdP {
  const bf16 *q, *k, *v, *dout;
  const float *lse, *delta;  // [B, H, Lq]; lse in base 2 (attn_fwd)
  float* ws;                 // [B, H, nsplit, Lq, D] fp32 partial dQ (unscaled)
  bf16 *dk, *dv;             // [B, Lnew, ...]: gradients of the last Lnew key rows
  long ldq, ldk, ldv, ldo, lddk, lddv;
  long sqb, skb, svb, sob, sdkb, sdvb;
  long Lq, Lkv, Lnew;
  int H, nsplit;
  float scale, scale_log2;
};

// rows r0 .. r0 + ROWS - 1 of a [*, D] bf16 matrix (zeros from row rend on) -> D / 64 sub-tiles of
// ROWS x 128-B rows, chunk-swizzled for both row and transposed fragment reads (swz_dual)
template <int ROWS, int D>
DEV void stage_rows(char* lds, const bf16* base, long ld, long r0, long rend) {
  constexpr int CPR = D / 8;  // 16-B chunks per row
  constexpr int N = ROWS * CPR / 256;
  bf16x8 r[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int idx = threadIdx.x + 256 * i;
    const long row = r0 + idx / CPR;
    r[i] = row < rend ? *(const bf16x8*)(base + row * ld + (idx % CPR) * 8) : bf16x8{};
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int idx = threadIdx.x + 256 * i;
    const int row = idx / CPR, ch = idx % CPR;
    *(bf16x8*)(lds + (ch >> 3) * ROWS * 128 + row * 128 + (((ch & 7) ^ swz_dual(row)) << 4)) = r[i];
  }
}

template <int D>
__global__ __launch_bounds__(256, 2) void attn_decode_bwd_k(DecBwdP p) {  // 64 KiB LDS: two per CU
  using C = DecBwdCfg<D>;
  constexpr int KS = C::KS, NKD = C::NKD, NDS = C::NDS, NKT = C::NKT;
  __shared__ __attribute__((aligned(16))) char smem[C::SMEM];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int split = blockIdx.x, head = blockIdx.y;
  const long b = blockIdx.z;
  const long k0 = (long)split * KS;
  const long kend = k0 + KS < p.Lkv ? k0 + KS : p.Lkv;

  const bf16* Q = p.q + b * p.sqb + head * D;
  const bf16* K = p.k + b * p.skb + head * D;
  const bf16* V = p.v + b * p.svb + head * D;
  const bf16* dO = p.dout + b * p.sob + head * D;
  const float* LSE = p.lse + (b * p.H + head) * p.Lq;
  const float* DLT = p.delta + (b * p.H + head) * p.Lq;

  // ---------------------------------------------------------------- phase 1: partial dQ of this split
  {
    char* lk = smem;
    char* lv = smem + C::NSUB * C::SUBK;
    stage_rows<KS, D>(lk, K, p.ldk, k0, p.Lkv);
    stage_rows<KS, D>(lv, V, p.ldv, k0, p.Lkv);
    __syncthreads();
    const int nkc = (int)((kend - k0 + 31) / 32);
    const int nqt = (int)((p.Lq + 15) / 16);
    float* WS = p.ws + (((b * p.H + head) * p.nsplit + split) * p.Lq) * D;
    for (int qt = w; qt < nqt; qt += 4) {
      const long my_q = 16L * qt + c;
      const bool qok = my_q < p.Lq;
      bf16x8 qf[NKD], df[NKD];  // this lane's query (column c) as B operands
#pragma unroll
      for (int kd = 0; kd < NKD; ++kd) {
        qf[kd] = qok ? *(const bf16x8*)(Q + my_q * p.ldq + 32 * kd + 8 * g) : bf16x8{};
        df[kd] = qok ? *(const bf16x8*)(dO + my_q * p.ldo + 32 * kd + 8 * g) : bf16x8{};
      }
      const float lse_q = qok ? LSE[my_q] : INFINITY;  // a query past Lq: P = 0
      const float dl_q = qok ? DLT[my_q] : 0.f;
      f32x4 dq[NDS];
#pragma unroll
      for (int ds = 0; ds < NDS; ++ds) dq[ds] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int kc = 0; kc < nkc; ++kc) {
        f32x4 st[2], dp[2];  // rows = keys 32 kc + 16 kk + 4 g + r, column = query c
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) st[kk] = dp[kk] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kd = 0; kd < NKD; ++kd)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            const bf16x8 ak = frag_row16<SW_DUAL>(lk + (kd >> 1) * C::SUBK, 32 * kc + 16 * kk, kd & 1, lane);
            const bf16x8 av = frag_row16<SW_DUAL>(lv + (kd >> 1) * C::SUBK, 32 * kc + 16 * kk, kd & 1, lane);
            st[kk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ak, qf[kd], st[kk], 0, 0, 0);
            dp[kk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, df[kd], dp[kk], 0, 0, 0);
          }
        const long kb0 = k0 + 32 * kc + 4 * g;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float pv = __builtin_amdgcn_exp2f(st[kk][r] * p.scale_log2 - lse_q);
            pv = kb0 + 16 * kk + r < p.Lkv ? pv : 0.f;  // keys past Lkv (zero rows in LDS)
            dp[kk][r] = pv * (dp[kk][r] - dl_q);
          }
        const bf16x8 sf = pack_perm(dp[0], dp[1]);
#pragma unroll
        for (int ds = 0; ds < NDS; ++ds) {
          const bf16x8 akt = frag_tr16<SW_DUAL>(lk + (ds >> 2) * C::SUBK, 32 * kc, ds & 3, lane);
          dq[ds] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(akt, sf, dq[ds], 0, 0, 0);
        }
      }
      // dQ^T tiles: this lane holds d = 16 ds + 4 g + r of query c
      if (qok) {
#pragma unroll
        for (int ds = 0; ds < NDS; ++ds) *(f32x4*)(WS + my_q * D + 16 * ds + 4 * g) = dq[ds];
      }
    }
  }

  // ---------------------------------------------------------------- phase 2: dK, dV of the new keys
  const long first_new = p.Lkv - p.Lnew;
  const long nlo = k0 > first_new ? k0 : first_new;
  if (nlo >= kend) return;  // workgroup-uniform

  // a pass = 64 NKT new keys (one frame of 64 is one pass of one tile per wave); the accumulators of a
  // pass stay in registers over the sweep of the query tiles
  for (long pbase = nlo; pbase < kend; pbase += 64 * NKT) {
    long my_k[NKT];
    bf16x8 kf[NKT][NKD], vf[NKT][NKD];  // this lane's keys (column c of the wave's 16-key tiles w + 4 i)
    f32x4 dk[NKT][NDS], dv[NKT][NDS];
#pragma unroll
    for (int i = 0; i < NKT; ++i) {
      my_k[i] = pbase + 16 * (w + 4 * i) + c;
      const bool kok = my_k[i] < kend;
#pragma unroll
      for (int ks = 0; ks < NKD; ++ks) {
        kf[i][ks] = kok ? *(const bf16x8*)(K + my_k[i] * p.ldk + 32 * ks + 8 * g) : bf16x8{};
        vf[i][ks] = kok ? *(const bf16x8*)(V + my_k[i] * p.ldv + 32 * ks + 8 * g) : bf16x8{};
      }
#pragma unroll
      for (int ds = 0; ds < NDS; ++ds) dk[i][ds] = dv[i][ds] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    char* lq = smem;
    char* ld = smem + C::NSUB * C::SUBQ;
    float* l2 = (float*)(smem + 2 * C::NSUB * C::SUBQ);
    float* dlt = l2 + 64;
    for (long q0 = 0; q0 < p.Lq; q0 += 64) {
      __syncthreads();  // every wave is done with the image this tile replaces
      stage_rows<64, D>(lq, Q, p.ldq, q0, p.Lq);
      stage_rows<64, D>(ld, dO, p.ldo, q0, p.Lq);
      if (threadIdx.x < 64) {
        const long qi = q0 + threadIdx.x;
        l2[threadIdx.x] = qi < p.Lq ? LSE[qi] : INFINITY;  // a query past Lq: P = 0
        dlt[threadIdx.x] = qi < p.Lq ? DLT[qi] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NKT; ++i) {
        if (pbase + 16 * (w + 4 * i) < kend) {  // wave-uniform
#pragma unroll
          for (int qb = 0; qb < 2; ++qb) {
            if (q0 + 32 * qb < p.Lq) {
              f32x4 st[2], dp[2];  // rows = queries 32 qb + 16 qs + 4 g + r, column = key c
#pragma unroll
              for (int qs = 0; qs < 2; ++qs) st[qs] = dp[qs] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int ks = 0; ks < NKD; ++ks)
#pragma unroll
                for (int qs = 0; qs < 2; ++qs) {
                  const bf16x8 aq = frag_row16<SW_DUAL>(lq + (ks >> 1) * C::SUBQ, 32 * qb + 16 * qs, ks & 1, lane);
                  const bf16x8 ad = frag_row16<SW_DUAL>(ld + (ks >> 1) * C::SUBQ, 32 * qb + 16 * qs, ks & 1, lane);
                  st[qs] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq, kf[i][ks], st[qs], 0, 0, 0);
                  dp[qs] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ad, vf[i][ks], dp[qs], 0, 0, 0);
                }
#pragma unroll
              for (int qs = 0; qs < 2; ++qs) {
                const int rowb = 32 * qb + 16 * qs + 4 * g;
                const f32x4 L = *(const f32x4*)(l2 + rowb);
                const f32x4 Dl = *(const f32x4*)(dlt + rowb);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const float pv = __builtin_amdgcn_exp2f(st[qs][r] * p.scale_log2 - L[r]);
                  st[qs][r] = pv;
                  dp[qs][r] = pv * (dp[qs][r] - Dl[r]);
                }
              }
              const bf16x8 pf = pack_perm(st[0], st[1]), sf = pack_perm(dp[0], dp[1]);
#pragma unroll
              for (int ds = 0; ds < NDS; ++ds) {
                const bf16x8 ado = frag_tr16<SW_DUAL>(ld + (ds >> 2) * C::SUBQ, 32 * qb, ds & 3, lane);
                const bf16x8 aqt = frag_tr16<SW_DUAL>(lq + (ds >> 2) * C::SUBQ, 32 * qb, ds & 3, lane);
                dv[i][ds] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ado, pf, dv[i][ds], 0, 0, 0);
                dk[i][ds] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aqt, sf, dk[i][ds], 0, 0, 0);
              }
            }
          }
        }
      }
    }
    // dK^T, dV^T tiles: this lane holds d = 16 ds + 4 g + r of its keys
#pragma unroll
    for (int i = 0; i < NKT; ++i) {
      if (my_k[i] >= kend) continue;
      const long row = my_k[i] - first_new;
      bf16* pk = p.dk + b * p.sdkb + row * p.lddk + head * D + 4 * g;
      bf16* pv = p.dv + b * p.sdvb + row * p.lddv + head * D + 4 * g;
#pragma unroll
      for (int ds = 0; ds < NDS; ++ds) {
        bf16x4 a4, b4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a4[e] = (bf16)(dk[i][ds][e] * p.scale);
          b4[e] = (bf16)dv[i][ds][e];
        }
        *(bf16x4*)(pk + 16 * ds) = a4;
        *(bf16x4*)(pv + 16 * ds) = b4;
      }
    }
  }
}

// dq[b, q, head D + d] = bf16(scale * sum_s ws[b, head, s, q, d]), s = 0 .. nsplit - 1 in order
__global__ __launch_bounds__(256) void attn_decode_bwd_reduce_k(const float* __restrict__ ws, bf16* dq, long lddq,
                                                                long sdqb, long total, int H, long Lq, int D,
                                                                int nsplit, float scale) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int d4 = D / 4;
  const int dc = (int)(idx % d4);
  const long q = (idx / d4) % Lq;
  const long bh = idx / d4 / Lq;
  const float* src = ws + ((bh * nsplit) * Lq + q) * D + 4 * dc;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < nsplit; ++s) {
    const f32x4 v = *(const f32x4*)(src + (long)s * Lq * D);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += v[e];
  }
  bf16x4 o4;
#pragma unroll
  for (int e = 0; e < 4; ++e) o4[e] = (bf16)(acc[e] * scale);
  *(bf16x4*)(dq + (bh / H) * sdqb + q * lddq + (bh % H) * (long)D + 4 * dc) = o4;
}

}  // namespace

extern "C" long owlk_attn_decode_bwd_ws_bytes(long B, int H, long Lq, long Lkv, int head_dim) {
  if ((head_dim != 64 && head_dim != 128) || B <= 0 || H <= 0 || Lq <= 0 || Lkv <= 0) return 0;
  const long n = B * H * (long)splits_of(Lkv, head_dim) * Lq * head_dim * 4;
  return (n + 255) / 256 * 256;
}

extern "C" int owlk_attn_decode_bwd(const void* q, long ldq, long sqb, const void* k, long ldk, long skb,
                                    const void* v, long ldv, long svb, const void* dout, long ldo, long sob,
                                    const float* lse, const float* delta, void* dq, long lddq, long sdqb,
                                    void* dk_new, long lddk, long sdkb, void* dv_new, long lddv, long sdvb, long B,
                                    int H, long Lq, long Lkv, long Lnew, int head_dim, float scale, void* ws,
                                    long ws_bytes, void* stream) {
  OWLK_REQUIRE(head_dim == 64 || head_dim == 128, "attn_decode_bwd: head_dim %d not built (64, 128)", head_dim);
  OWLK_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535 && Lq > 0 && Lkv > 0 && Lq < (1L << 31) &&
                   Lkv < (1L << 31),
               "attn_decode_bwd: bad sizes B=%ld H=%d Lq=%ld Lkv=%ld", B, H, Lq, Lkv);
  OWLK_REQUIRE(Lnew >= 0 && Lnew <= Lkv, "attn_decode_bwd: Lnew=%ld must lie in 0 .. Lkv=%ld", Lnew, Lkv);
  OWLK_REQUIRE(q && k && v && dout && dq && lse && delta, "attn_decode_bwd: null operand");
  OWLK_REQUIRE(Lnew == 0 || (dk_new && dv_new), "attn_decode_bwd: dk_new / dv_new needed for Lnew=%ld", Lnew);
  uintptr_t al = (uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)dout | (uintptr_t)dq;
  if (Lnew > 0) al |= (uintptr_t)dk_new | (uintptr_t)dv_new;
  OWLK_REQUIRE(al % 16 == 0 && ((uintptr_t)lse | (uintptr_t)delta) % 4 == 0,
               "attn_decode_bwd: operands must be 16-byte aligned");
  const long hd = (long)H * head_dim;
  const long lds_[5] = {ldq, ldk, ldv, ldo, lddq};
  for (long ld : lds_)
    OWLK_REQUIRE(ld >= hd && ld % 8 == 0 && ld < (1L << 31),
                 "attn_decode_bwd: row stride %ld must be a multiple of 8 in H*D=%ld .. 2^31-1", ld, hd);
  if (Lnew > 0)
    OWLK_REQUIRE(lddk >= hd && lddk % 8 == 0 && lddk < (1L << 31) && lddv >= hd && lddv % 8 == 0 &&
                     lddv < (1L << 31),
                 "attn_decode_bwd: row strides %ld, %ld of dk_new, dv_new must be multiples of 8 in H*D=%ld .. 2^31-1",
                 lddk, lddv, hd);
  OWLK_REQUIRE(B == 1 || ((sqb | skb | svb | sob | sdqb) % 8 == 0 && (Lnew == 0 || (sdkb | sdvb) % 8 == 0)),
               "attn_decode_bwd: batch strides must be multiples of 8");
  const long need = owlk_attn_decode_bwd_ws_bytes(B, H, Lq, Lkv, head_dim);
  OWLK_REQUIRE(ws && ws_bytes >= need, "attn_decode_bwd: workspace of %ld bytes, %ld needed", ws ? ws_bytes : 0L,
               need);
  OWLK_REQUIRE((uintptr_t)ws % 256 == 0, "attn_decode_bwd: workspace must be 256-byte aligned");
  const long total = B * H * Lq * (head_dim / 4);
  OWLK_REQUIRE((total + 255) / 256 < (1L << 31), "attn_decode_bwd: B*H*Lq=%ld too large", B * H * Lq);

  DecBwdP p;
  p.q = (const bf16*)q; p.k = (const bf16*)k; p.v = (const bf16*)v; p.dout = (const bf16*)dout;
  p.lse = lse; p.delta = delta;
  p.ws = (float*)ws;
  p.dk = (bf16*)dk_new; p.dv = (bf16*)dv_new;
  p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo; p.lddk = lddk; p.lddv = lddv;
  p.sqb = sqb; p.skb = skb; p.svb = svb; p.sob = sob; p.sdkb = sdkb; p.sdvb = sdvb;
  p.Lq = Lq; p.Lkv = Lkv; p.Lnew = Lnew;
  p.H = H;
  p.nsplit = splits_of(Lkv, head_dim);
  p.scale = scale;
  p.scale_log2 = scale * LOG2E;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)p.nsplit, (unsigned)H, (unsigned)B);
  if (head_dim == 64)
    hipLaunchKernelGGL(attn_decode_bwd_k<64>, grid, dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(attn_decode_bwd_k<128>, grid, dim3(256), 0, s, p);
  if (int e = owlk::check_launch("attn_decode_bwd")) return e;
  hipLaunchKernelGGL(attn_decode_bwd_reduce_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                     (const float*)ws, (bf16*)dq, lddq, sdqb, total, H, Lq, head_dim, p.nsplit, scale);
  return owlk::check_launch("attn_decode_bwd_reduce");
}
