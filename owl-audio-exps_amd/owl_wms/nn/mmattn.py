"""mmattn.py (reference: owl_wms/nn/mmattn.py:28-152) -- two-stream MMDiT on libowlk.

Per layer (``MMDiTBlockFn``, one autograd Function for the whole block, both modalities):
    h_s   = cond_adaln(x_s, scale_s, bias_s)            adaln_fwd    (video tpf 64, audio tpf 1)
    qkv_s = h_s Wqkv_s^T + b                            GEMM
    joint = frame_interleave(qkv_v, qkv_a)              frame_mux: frame f = [64 video | 1 audio]
    q, k  = rope(rms(q)), rope(rms(k))                  qk_rope_fwd  (OrthoRoPE table, 65-token frames)
    o     = attn(q, k, v)                               attn_fwd     (frame mask, tpf 65, local/global window)
    o_s   = frame_split(o)                              frame_mux
    x_s  += gate_s * (o_s Wout_s^T + b)                 GEMM + gate/residual epilogue
    x_s  += gate2_s * MLP_s(cond_adaln(x_s, ...))       adaln_fwd + GEMM(SiLU) + GEMM(gate/residual)
and the mirrored backward.  The modulation is shared by every layer (DiT-Air, mmattn.py:126-130,
148): each block returns its [B, F, 6d] modulation gradient in the reference's chunk order
(attn scale, bias, gate, mlp scale, bias, gate) and autograd sums them across layers.

The reference module imports a missing ``create_causal_block_mask``; its
mask is reconstructed as get_block_mask(n, tpf, window, no docs, q_offset, causal) -- a
FrameMask here.

KV cache (mmattn.py:46-72, decode / sampling, no grad): the new joint frame(s) are rotated at
offset = the layer's cached length, [cache | new] K/V are read in place (SingleKVCache.extend),
the cache is committed when updates are enabled, and the attention keeps the frame mask with
q_offset = the cached length (the reference's create_causal_block_mask(n_cached_tokens=offset)).
With MMDIT.enable_decoding() (off by default; the causal audio + video samplers switch it on around
their decode steps) a cached call at head_dim 64 takes MMDiTBlock._forward_decode: the rope kernel reads
the two qkv outputs and writes k / v straight into the cache (no interleave, no extend copies), and one
new frame runs the joint decode attention with the video / audio rows written apart (no split).
A RingKVCache past its context pass (sampling/stream.py AVFrameStream) takes MMDiTBlock._forward_ring_decode:
the same launch list on the two kernels' ring forms, the position read from the cache's device vector and
the new rows roped at the absolute offset.
"""
import torch
from torch import nn

from .. import kernels as K
from .attn import check_rope_rows
from .fused import (bf16_weight, bgrad_into, block_head_bwd, block_tail, block_tail_bwd, cond_silu, grad_done, linear,
                    wgrad_into)
from .mlp import MLP
from .rope import get_rope_cls

BF16 = torch.bfloat16


class MMGeometry:
    def __init__(self, n_heads, head_dim, n0, n1, mask, cos, sin):
        self.H, self.D, self.n0, self.n1, self.mask, self.cos, self.sin = n_heads, head_dim, n0, n1, mask, cos, sin


def _joint_views(j, n0, n1, cols):
    """The per-modality rows of a joint-sequence buffer j [F (n0 + n1), cols] as operands that
    libowlk reads / writes in place: the video rows as a frame-strided [F, n0, cols] view
    (kernels.frame_rows), the audio row of every frame as a plain strided [F, cols] view."""
    F_ = j.shape[0] // (n0 + n1)
    return K.frame_rows(j, n0, n1, 0, cols), j.view(F_, n0 + n1, cols)[:, n0, :]


def _in_place_ok(d, n0, n1, frames):
    """The joint layout is used in place (no frame_mux copies) where the video GEMMs tile by 256
    (owlk_gemm_frames): mmdit_v2 (d 1536, 8x8 latents + 1 audio token per frame), for more than
    four frames of video rows (fewer take the frame_mux path, as decode-sized GEMMs)."""
    return n0 == K.FRAME_ROWS and n1 == 1 and d % 256 == 0 and frames * n0 > 256


def _lane_ok(inplace, frames, n1):
    """The audio side stream only where its GEMMs (frames * n1 rows) stay off the decode plan, whose
    workspace counters are shared per device (kernels._decode_ws)."""
    return inplace and frames * n1 > 128


_AUDIO_STREAMS = {}


class _AudioLane:
    """The audio modality's per-block work (adaln, its 1,000-row GEMMs, gate / adaln backward) on a
    side HIP stream beside the video's: at mmdit_v2 the audio rows are 1/64 of the video's, so their
    GEMMs fill few CUs and run at a fifth of the video GEMMs' rate (3 % of the micro-step serially).
    fork(): the side stream waits for everything enqueued so far; join(): the caller's stream waits
    for the side stream.  Tensors the side stream allocates are marked for the caller's stream
    (record_stream), so the caching allocator never hands their blocks to later side-stream work while
    the caller's stream may still read them.  Serial (no side stream) for the frame_mux layout, while a
    profile window is open or a graph is being captured, or with OWLK_MMDIT_AUDIO_STREAM=0."""

    def __init__(self, device, enable):
        import os
        from .. import _lib
        self.main = torch.cuda.current_stream(device)
        self.side = None
        if enable and os.environ.get("OWLK_MMDIT_AUDIO_STREAM", "1") != "0" and not _lib.profiling() and \
                not torch.cuda.is_current_stream_capturing():
            self.side = _AUDIO_STREAMS.get(device)
            if self.side is None:
                self.side = _AUDIO_STREAMS[device] = torch.cuda.Stream(device=device)

    def fork(self):
        if self.side is not None:
            self.side.wait_stream(self.main)

    def join(self):
        if self.side is not None:
            self.main.wait_stream(self.side)

    def on(self, s):
        """context for modality s's work: the side stream for audio (s = 1)"""
        import contextlib
        return torch.cuda.stream(self.side) if (s == 1 and self.side is not None) else contextlib.nullcontext()

    def mark(self, ts):
        if self.side is not None:
            for t in ts:
                if isinstance(t, torch.Tensor):
                    t.record_stream(self.main)


def _modality_slots(s):
    """Where modality s's parameters stand among MMDiTBlockFn's sixteen (*w, and the gradients it
    returns): its (qkv weight, bias), and its tail (out weight, bias, fc1 weight, bias, fc2 weight,
    bias) in fused.block_tail's order.  *w = the two qkv pairs, the two out pairs, the two MLPs' four."""
    return (2 * s, 2 * s + 1), (4 + 2 * s, 5 + 2 * s, 8 + 4 * s, 9 + 4 * s, 10 + 4 * s, 11 + 4 * s)


def _modality_params(w, s):
    qkv, tail = _modality_slots(s)
    return tuple(w[i] for i in qkv), tuple(w[i] for i in tail)


def _cast_weights(ws):
    """Refresh the cached bf16 copies of ws (a cast after an optimizer step) on the caller's stream,
    before a lane fork: the block functions then find them cached on whichever stream they run."""
    for p in ws:
        bf16_weight(p)


class MMDiTBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, x1, c0, c1, geo, *w):
        B, T0, d = x0.shape
        H, D, n0, n1 = geo.H, geo.D, geo.n0, geo.n1
        nf = B * (T0 // n0)
        T = (T0 // n0) * (n0 + n1)
        xs = (x0.reshape(-1, d), x1.reshape(-1, d))
        ms = (c0.reshape(nf, 6 * d), c1.reshape(nf, 6 * d))
        ns = (n0, n1)
        prm = [_modality_params(w, s) for s in range(2)]  # ((wqkv, bqkv), tail) per modality
        inplace = _in_place_ok(d, n0, n1, nf)
        lane = _AudioLane(x0.device, _lane_ok(inplace, nf, n1))
        h1, r1, qkv = [None, None], [None, None], [None, None]
        if inplace:  # each modality's qkv projection writes its rows of the joint frames directly
            qkvj = torch.empty(B * T, 3 * d, device=x0.device, dtype=BF16)
            qkv_dst = _joint_views(qkvj, n0, n1, 3 * d)
        wq = [bf16_weight(prm[s][0][0]) for s in range(2)]
        lane.fork()
        for s in (1, 0):  # audio first: its launches go to the side stream, then the video's run beside
            with lane.on(s):
                h1[s], r1[s] = K.adaln_fwd(xs[s], ms[s][:, :d], ms[s][:, d:2 * d], ns[s])
                qkv[s] = K.gemm(h1[s], wq[s], bias=prm[s][0][1], out=qkv_dst[s] if inplace else None)
        lane.mark(h1[1:] + r1[1:])
        lane.join()
        if not inplace:
            qkvj = K.frame_interleave(qkv[0], qkv[1], n0, n1)
        del qkv
        qkr, rq = K.qk_rope_fwd(qkvj, H, D, geo.cos, geo.sin, 0, T)
        q3, k3 = qkr.view(B, T, 2 * d)[:, :, :d], qkr.view(B, T, 2 * d)[:, :, d:]
        o, lse = K.attn_fwd(q3, k3, qkvj.view(B, T, 3 * d)[:, :, 2 * d:], H, D, geo.mask,
                            score_bound=K.qk_norm_bound(D))
        os_ = _joint_views(o.view(B * T, d), n0, n1, d) if inplace else K.frame_split(o.view(B * T, d), n0, n1)
        saved, outs = [None, None], [None, None]
        _cast_weights(p for s in range(2) for p in prm[s][1][0::2])
        lane.fork()
        for s in (1, 0):
            with lane.on(s):
                outs[s], acts = block_tail(os_[s], xs[s], ms[s], ns[s], prm[s][1])
                saved[s] = [xs[s], ms[s], h1[s], r1[s], *acts]  # acts: y1, x1, h2, r2, a_pre, a, y2
        lane.mark(saved[1][4:] + [outs[1]])
        lane.join()
        ctx.save_for_backward(qkvj, qkr, rq, o, lse, *saved[0], *saved[1], *w)
        ctx.geo, ctx.dims = geo, (B, T0, x1.shape[1], d, T, nf)
        ctx.params = w  # the Parameters themselves: their GradReducer bucket views are the gradient sinks
        return outs[0].view(B, T0, d), outs[1].view(B, x1.shape[1], d)

    @staticmethod
    def backward(ctx, dout0, dout1):
        qkvj, qkr, rq, o, lse = ctx.saved_tensors[:5]
        st = [ctx.saved_tensors[5:16], ctx.saved_tensors[16:27]]
        geo = ctx.geo
        B, T0, T1, d, T, nf = ctx.dims
        H, D, n0, n1 = geo.H, geo.D, geo.n0, geo.n1
        ns = (n0, n1)
        dW = [None] * 16  # in the order of *w; None where the gradient went into the parameter's bucket view
        prm = [_modality_params(ctx.params, s) for s in range(2)]
        slots = [_modality_slots(s) for s in range(2)]
        # parameters whose bucket view is complete (fused.wgrad_into's done): a write may be on the side
        # stream, so the reducer hears of it on the main stream after the join
        done = []

        def report():  # after a lane join: every write above is ordered before the main stream's next work
            for q in done:
                grad_done(q)
            done.clear()

        dcs = [torch.empty(nf, 6 * d, device=dout0.device, dtype=BF16) for _ in range(2)]  # d mods, bf16
        douts = (dout0.reshape(-1, d).to(BF16).contiguous(), dout1.reshape(-1, d).to(BF16).contiguous())
        inplace = _in_place_ok(d, n0, n1, nf)
        lane = _AudioLane(o.device, _lane_ok(inplace, nf, n1))
        if inplace:  # per-modality views of the joint o, and the joint dO the two dX GEMMs write into
            os_ = _joint_views(o.view(B * T, d), n0, n1, d)
            do = torch.empty(B * T, d, device=o.device, dtype=BF16)
            do_dst = _joint_views(do, n0, n1, d)
        else:
            os_ = K.frame_split(o.view(B * T, d), n0, n1)
        dos, dx1s = [None, None], [None, None]
        _cast_weights(p for s in range(2) for p in prm[s][1][0::2])
        lane.fork()
        for s in (1, 0):
            with lane.on(s):
                tail = prm[s][1]
                dx1s[s], dy1, grads = block_tail_bwd(douts[s], st[s][0], st[s][1], dcs[s], ns[s], tail, st[s][4:],
                                                     done.append)
                # ---- attention output projection
                dos[s] = K.gemm(dy1, bf16_weight(tail[0]), b_trans=True, out=do_dst[s] if inplace else None)
                dwout = wgrad_into(tail[0], dy1, os_[s], done.append)
                for i, g in zip(slots[s][1], (dwout,) + grads):  # dwout, dbout, dw1, db1, dw2, db2
                    dW[i] = g
        lane.mark([dW[i] for i in slots[1][1]] + [dx1s[1]] + [dos[1]])  # audio's
        lane.join()
        report()
        del os_
        if not inplace:
            do = K.frame_interleave(dos[0], dos[1], n0, n1)
        del dos
        dqkvj = torch.empty(B * T, 3 * d, device=o.device, dtype=BF16)
        dqkr = torch.empty(B * T, 2 * d, device=o.device, dtype=BF16)
        q3, k3 = qkr.view(B, T, 2 * d)[:, :, :d], qkr.view(B, T, 2 * d)[:, :, d:]
        dq3, dk3 = dqkr.view(B, T, 2 * d)[:, :, :d], dqkr.view(B, T, 2 * d)[:, :, d:]
        K.attn_bwd(q3, k3, qkvj.view(B, T, 3 * d)[:, :, 2 * d:], o.view(B, T, d), do.view(B, T, d), lse, H, D,
                   geo.mask, dq3, dk3, dqkvj.view(B, T, 3 * d)[:, :, 2 * d:])
        del do
        K.qk_rope_bwd(dqkr, qkvj, rq, H, D, geo.cos, geo.sin, dqkvj, 0, T)
        del dqkr
        # the per-modality qkv gradients: views of the joint rows (in place) or split copies
        dqkv = _joint_views(dqkvj, n0, n1, 3 * d) if inplace else K.frame_split(dqkvj, n0, n1)
        dxs = [None, None]
        _cast_weights(prm[s][0][0] for s in range(2))
        lane.fork()
        for s in (1, 0):
            with lane.on(s):
                xs, ms, h1, r1 = st[s][:4]
                (wqkv, bqkv), (iw, ib) = prm[s][0], slots[s][0]
                dW[ib] = bgrad_into(bqkv, dqkv[s], done.append)
                dxs[s], dW[iw] = block_head_bwd(dqkv[s], h1, xs, r1, ms, dcs[s], ns[s], wqkv, dx1s[s], done.append)
        lane.mark([dW[i] for i in slots[1][0]] + [dxs[1], dcs[1]])
        lane.join()
        report()
        return (dxs[0].view(B, T0, d), dxs[1].view(B, T1, d), dcs[0].view(B, nf // B, 6 * d),
                dcs[1].view(B, nf // B, 6 * d), None, *dW)


class MMAttn(nn.Module):
    """mmattn.py:28-86 -- parameters / keys of the reference; compute lives in MMDiTBlockFn."""

    def __init__(self, config, layer_idx, rope=None):
        super().__init__()
        self.config = config
        self.layer_idx = layer_idx
        self.n_heads = config.n_heads
        self.tok_per_frame_mod = [config.sample_size ** 2, 1]
        self.qkv_projs = nn.ModuleList([nn.Linear(config.d_model, 3 * config.d_model) for _ in range(2)])
        self.out_projs = nn.ModuleList([nn.Linear(config.d_model, config.d_model) for _ in range(2)])
        object.__setattr__(self, "rope", rope if rope is not None else
                           get_rope_cls(getattr(config, "rope_impl", "ortho"))(config))


class MMDiTBlock(nn.Module):
    # _forward_decode's single-frame attention: the joint decode kernel (False: the masked attn_fwd +
    # frame_split after the joint-frame rope kernel; tools/av_decode_bench.py times the two apart)
    joint_attention = True

    def __init__(self, config, layer_idx, rope=None):
        super().__init__()
        self.config = config
        self.attn = MMAttn(config, layer_idx, rope)
        self.mlps = nn.ModuleList([MLP(config) for _ in range(2)])
        self.decoding = False  # MMDIT.enable_decoding: the fused cache path (_forward_decode)

    def forward(self, x0, x1, cond0, cond1, block_mask=None, kv_cache=None):
        if kv_cache is not None:
            with torch.no_grad():
                # a SlotRingKVCache (sampling/stream_pool.py AVStreamPool) decodes whatever its slots' offsets
                if getattr(kv_cache, "ring", False) and (kv_cache.get_offset(self.attn.layer_idx) > 0 or
                                                         getattr(kv_cache, "n_slots", None) is not None):
                    return self._forward_ring_decode(x0, x1, cond0, cond1, block_mask, kv_cache)
                if self.decoding and self._decode_ok(block_mask, kv_cache):
                    return self._forward_decode(x0, x1, cond0, cond1, block_mask, kv_cache)
                return self._forward_cached(x0, x1, cond0, cond1, block_mask, kv_cache)
        cfg, a = self.config, self.attn
        H = cfg.n_heads
        n0 = cfg.sample_size ** 2
        geo = MMGeometry(H, cfg.d_model // H, n0, 1, block_mask, a.rope.cos, a.rope.sin)
        ws = [None] * 16
        for s in range(2):
            qkv_at, tail_at = _modality_slots(s)
            for i, p in zip(qkv_at + tail_at, self.qkv_params(s) + self.tail_params(s)):
                ws[i] = p
        return MMDiTBlockFn.apply(x0.to(BF16).contiguous(), x1.to(BF16).contiguous(), cond0, cond1, geo, *ws)

    def qkv_params(self, s):
        return self.attn.qkv_projs[s].weight, self.attn.qkv_projs[s].bias

    def tail_params(self, s):
        """(wout, bout, w1, b1, w2, b2) of modality s: its parameters after the attention (fused.block_tail)"""
        o, m = self.attn.out_projs[s], self.mlps[s]
        return o.weight, o.bias, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias

    def _cached_dims(self, x0):
        """(d, H, D, n0, n1, B, frames, joint rows per batch row) of a cached forward of x0 [B, frames n0, d]"""
        cfg = self.config
        d, H, n0, n1 = cfg.d_model, cfg.n_heads, cfg.sample_size ** 2, 1
        nf = x0.shape[1] // n0
        return d, H, d // H, n0, n1, x0.shape[0], nf, nf * (n0 + n1)

    def _cached_head(self, x0, x1, cond0, cond1):
        """What every cached forward opens with: per modality the bf16 rows xs, the modulation rows ms and
        the qkv GEMM's output of the AdaLN-ed rows (AdaLN x 2, qkv GEMM x 2)."""
        d, n0 = self.config.d_model, self.config.sample_size ** 2
        xs = (x0.reshape(-1, d).to(BF16).contiguous(), x1.reshape(-1, d).to(BF16).contiguous())
        ms = (cond0.reshape(-1, 6 * d), cond1.reshape(-1, 6 * d))
        qkv = []
        for s, n in enumerate((n0, 1)):
            h, _ = K.adaln_fwd(xs[s], ms[s][:, :d], ms[s][:, d:2 * d], n)
            wqkv, bqkv = self.qkv_params(s)
            qkv.append(K.gemm(h, bf16_weight(wqkv), bias=bqkv))
        return xs, ms, qkv

    def _cached_tail(self, os_, xs, ms, B):
        """What every cached forward closes with: each modality's block_tail on its attention rows os_[s]
        (4 launches each) -> the block's outputs [B, frames n0, d], [B, frames, d]."""
        d, n0 = self.config.d_model, self.config.sample_size ** 2
        outs = [block_tail(os_[s], xs[s], ms[s], n, self.tail_params(s), save=False)[0] for s, n in enumerate((n0, 1))]
        return outs[0].view(B, -1, d), outs[1].view(B, -1, d)

    def _forward_cached(self, x0, x1, cond0, cond1, block_mask, kv_cache):
        """MMDiTBlock.forward (mmattn.py:98-114) with MMAttn's cache path (mmattn.py:46-72)."""
        a = self.attn
        d, H, D, n0, n1, B, nf, T = self._cached_dims(x0)
        xs, ms, qkv = self._cached_head(x0, x1, cond0, cond1)
        qkvj = K.frame_interleave(qkv[0], qkv[1], n0, n1)
        del qkv
        li = a.layer_idx
        offset = kv_cache.length_at(li)
        qkr, _ = K.qk_rope_fwd(qkvj, H, D, a.rope.cos, a.rope.sin, offset, T)
        q = qkr.view(B, T, 2 * d)[:, :, :d]
        k = qkr.view(B, T, 2 * d)[:, :, d:]
        v = qkvj.view(B, T, 3 * d)[:, :, 2 * d:]
        if offset > 0:
            if kv_cache.noise_caches == 0.0 and hasattr(kv_cache, "extend"):
                k, v = kv_cache.extend(li, k, v)
            else:
                old_k, old_v = kv_cache.get(li)
                k, v = torch.cat([old_k, k], dim=1), torch.cat([old_v, v], dim=1)
        if kv_cache.should_update:
            kv_cache.update(k, v, li)
        mask = block_mask if block_mask is not None else K.FrameMask(1, None, False, 0, None)
        o, _ = K.attn_fwd(q, k, v, H, D, mask, score_bound=K.qk_norm_bound(D))
        return self._cached_tail(K.frame_split(o.view(B * T, d), n0, n1), xs, ms, B)

    def _decode_ok(self, block_mask, kv_cache):
        """The fused decode path's cases (MMDIT.enable_decoding): head_dim 64, the causal frame mask, a
        cache read as stored with slots to write into."""
        cfg = self.config
        return cfg.d_model // cfg.n_heads == 64 and block_mask is not None and block_mask.causal and \
            block_mask.arrays is None and kv_cache.noise_caches == 0.0 and hasattr(kv_cache, "extend_slots") and \
            not getattr(kv_cache, "ring", False)  # a ring's new rows may wrap: no slot views (_forward_ring_decode)

    def _forward_decode(self, x0, x1, cond0, cond1, block_mask, kv_cache):
        """_forward_cached with the joint frames never assembled (MMDIT.enable_decoding): the rope kernel
        reads the two qkv GEMM outputs and writes q, and k / v straight into the cache's slots
        (kernels.mm_qk_rope_fwd_kv: no frame_interleave, no extend copies; the same q, k, v bit for bit).
        One new frame then takes the joint decode attention (kernels.attn_decode_joint_fwd: unmasked over
        the [cache | new] rows the frame mask allows -- all of them, the last `window` frames on a windowed
        layer -- with the video / audio rows written apart, no frame_split); several frames keep the masked
        attn_fwd and are bit-identical to _forward_cached.  14 launches per block and decode step against
        18: AdaLN x 2, qkv GEMM x 2, rope, attention, block_tail x 2 (4 each)."""
        a = self.attn
        d, H, D, n0, n1, B, nf, T = self._cached_dims(x0)
        xs, ms, qkv = self._cached_head(x0, x1, cond0, cond1)
        li = a.layer_idx
        offset = kv_cache.length_at(li)
        assert block_mask.q_offset == offset and block_mask.tpf == n0 + n1, "the frame mask describes this cache"
        q = torch.empty(B, T, d, device=x0.device, dtype=BF16)
        ks, vs = kv_cache.extend_slots(li, T, q)
        K.mm_qk_rope_fwd_kv(qkv[0], qkv[1], B, nf, n0, n1, H, D, a.rope.cos, a.rope.sin, offset, q, ks, vs)
        del qkv
        k, v = kv_cache.extended(li, T)
        if kv_cache.should_update:
            kv_cache.update(k, v, li)  # the rows are in place: committed without a copy
        if nf == 1 and self.joint_attention and K.decode_joint_supported(D, n0, n1) and K.qk_norm_bound(D) > 0.0:
            if block_mask.window:  # |frame_q - frame_kv| < window: the last `window` frames, this one included
                w = int(block_mask.window) * (n0 + n1)
                k, v = k[:, -w:], v[:, -w:]
            os_ = K.attn_decode_joint_fwd(q, k, v, H, D, n0, n1, score_bound=K.qk_norm_bound(D))[:2]
        else:
            o, _ = K.attn_fwd(q, k, v, H, D, block_mask, score_bound=K.qk_norm_bound(D))
            os_ = K.frame_split(o.view(B * T, d), n0, n1)
        return self._cached_tail(os_, xs, ms, B)

    def _forward_ring_decode(self, x0, x1, cond0, cond1, block_mask, kv_cache):
        """One new joint frame against a RingKVCache (sampling/stream.py AVFrameStream): _forward_decode's
        launch list -- AdaLN x 2, qkv GEMM x 2, rope, joint attention, block_tail x 2 -- on the ring forms of
        the two joint-frame kernels (kernels.mm_qk_rope_fwd_kv_ring, kernels.attn_decode_joint_ring_fwd).
        They read {start, cached tokens, rope offset} from the cache's device vector, so nothing here
        depends on a host position and a captured step stays valid across frames, wraps and rebases.
        The new rows are roped at the ABSOLUTE offset (the vector's third word), not at the cached length
        _forward_cached / _forward_decode use as mmattn.py:60-62 does: after an eviction the cached length
        points at positions live keys already hold.
        A SlotRingKVCache (sampling/stream_pool.py AVStreamPool) takes the two kernels' slot forms: one state
        row {start, cached, offset, live} per session, batch row b on row b mod n_slots."""
        a = self.attn
        d, H, D, n0, n1, B, nf, T = self._cached_dims(x0)
        if nf != 1 or D != 64 or kv_cache.dev is None or kv_cache.noise_caches != 0.0 or \
                not K.decode_joint_supported(D, n0, n1) or K.qk_norm_bound(D) <= 0.0:
            raise RuntimeError("a RingKVCache decodes one joint frame at a time on the device-state path (head_dim "
                               f"64, at most {K.JOINT_DECODE_ROWS} rows, noise_caches 0, enable_device_state() after "
                               f"the context pass; got {nf} frame(s) of {n0} + {n1} rows, head_dim {D}, noise_caches "
                               f"{kv_cache.noise_caches}, device state {'on' if kv_cache.dev is not None else 'off'})")
        xs, ms, qkv = self._cached_head(x0, x1, cond0, cond1)
        li = a.layer_idx
        kb, vb = kv_cache.bufs[li]
        q = torch.empty(B, T, d, device=x0.device, dtype=BF16)
        slots = getattr(kv_cache, "n_slots", None) is not None
        rope_kv, attend = (K.mm_qk_rope_fwd_kv_ring_slots, K.attn_decode_joint_ring_slots_fwd) if slots else \
            (K.mm_qk_rope_fwd_kv_ring, K.attn_decode_joint_ring_fwd)
        rope_kv(qkv[0], qkv[1], B, nf, n0, n1, H, D, a.rope.cos, a.rope.sin, kv_cache.dev, q, kb, vb)
        del qkv
        window = block_mask.window if block_mask is not None else None
        os_ = attend(q, kb, vb, H, D, n0, n1, kv_cache.dev, int(window) * T if window else 0,
                     score_bound=K.qk_norm_bound(D))[:2]
        if kv_cache.should_update:
            kv_cache.commit_device(li, T)
        return self._cached_tail(os_, xs, ms, B)


class MMDIT(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        assert config.tokens_per_frame == config.sample_size ** 2 + 1, "MMDiT frames are [p*p video | 1 audio]"
        self.rope = get_rope_cls(getattr(config, "rope_impl", "ortho"))(config)
        self.local_layers = [(i % 4 != 0) for i in range(config.n_layers)]
        self.blocks = nn.ModuleList([MMDiTBlock(config, i, self.rope) for i in range(config.n_layers)])
        self.cond_proj = nn.Sequential(nn.SiLU(), nn.Linear(config.d_model, config.d_model * 2 * 2 * 3))
        self.decoding = False

    def enable_decoding(self):
        """KV-cache forwards take MMDiTBlock._forward_decode where it applies (head_dim 64); off by
        default, and with it off every cached call is _forward_cached as before."""
        self.decoding = True
        for b in self.blocks:
            b.decoding = True

    def disable_decoding(self):
        self.decoding = False
        for b in self.blocks:
            b.decoding = False

    def get_block_mask(self, x0, x1, kv_cache, window_len):
        """mmattn.py:132-143: causal frame mask over [cache | new] (q_offset = cached tokens)."""
        if not self.config.causal:
            return K.FrameMask(self.config.tokens_per_frame, None, False, 0, None)
        offset = kv_cache.length_at(0) if kv_cache is not None else 0
        return K.FrameMask(self.config.tokens_per_frame, window_len, True, offset, None)

    def forward(self, x0, x1, cond, kv_cache=None):
        local_mask = self.get_block_mask(x0, x1, kv_cache, self.config.local_window)
        global_mask = self.get_block_mask(x0, x1, kv_cache, getattr(self.config, "global_window", None))
        lin = self.cond_proj[1]
        c = linear(cond_silu(cond), lin.weight, lin.bias)
        cond0, cond1 = c.chunk(2, dim=-1)
        ring = getattr(kv_cache, "ring", False)
        if ring:
            # the ring kernels read the position from the device and would only poison the rows with NaN:
            # check it on the host first, as the reference's short table slice fails (attn.check_rope_rows)
            check_rope_rows(self.rope, kv_cache.get_offset(0), x1.shape[1] * self.config.tokens_per_frame)
        for i, block in enumerate(self.blocks):
            x0, x1 = block(x0, x1, cond0, cond1, local_mask if self.local_layers[i] else global_mask, kv_cache)
        if ring and kv_cache.should_update:
            kv_cache.sync_device_state()  # every layer committed the frame
        return x0, x1
