"""kv_cache.py (reference: owl_wms/nn/kv_cache.py:5-104).

Same interface; K/V are kept token-major ``[B, T, H*D]`` bf16 (the layout the attention kernel
reads directly) instead of ``[B, H, T, D]``.
"""
import torch


def KVCache(config):
    if config.backbone in ("dit", "mmdit"):
        return SingleKVCache(config)
    raise ValueError(f"Invalid backbone: {config.backbone}")


class SingleKVCache:
    """Per layer a preallocated token-major K/V buffer ``[B, cap, d]`` with a live window
    ``[start, start + len)``.  ``extend`` writes a new frame's K/V behind the window and returns
    views of ``[cache | new]``: the decode step reads the cache in place instead of re-copying it
    with ``torch.cat`` per layer and step, and the addresses stay fixed while a frame is denoised
    (the sampler's HIP-graph replay relies on that)."""

    def __init__(self, config):
        self.config = config
        self.bufs = None
        self.device = "cuda"
        self.dtype = torch.bfloat16
        self.should_update = False
        self.noise_caches = 0.0
        self.offsets = [0] * config.n_layers
        self.start = [0] * config.n_layers
        self.len = [0] * config.n_layers
        self.dev = None  # device state {start, cached tokens, rope offset} (enable_device_state)

    def enable_device_state(self, capacity):
        """Decode with the cache position on the device: every layer's buffer is reserved for
        `capacity` tokens (no reallocation or compaction while sampling: fixed addresses), and the
        decode kernels read {start, cached tokens, rope offset} from an int64 device vector, so a
        HIP graph captured once serves every frame while the cache grows.  All layers advance
        together in decode, so one vector describes them all."""
        for i in range(self.config.n_layers):
            kb = self.bufs[i]
            assert kb is not None, "enable_device_state after the context pass"
            if kb[0].shape[1] < capacity:
                n, s = self.len[i], self.start[i]
                new = tuple(torch.empty(kb[0].shape[0], capacity, kb[0].shape[2], device=kb[0].device,
                                        dtype=kb[0].dtype) for _ in range(2))
                if n:
                    for dst, src in zip(new, (kb[0][:, s:s + n], kb[1][:, s:s + n])):
                        dst[:, :n].copy_(src)
                self.bufs[i], self.start[i] = new, 0
        self._create_device_state()

    def _create_device_state(self):
        self.dev = torch.zeros(4, dtype=torch.int64, device=self.bufs[0][0].device)
        self.sync_device_state()

    def _check_window(self, s, n):
        """the live window [s, s + n) lies in the buffers"""
        assert s + n <= self.bufs[0][0].shape[1]

    def sync_device_state(self):
        """host position -> the device vector (outside graph capture: an H2D copy)"""
        if self.dev is None:
            return
        st = {(self.start[i], self.len[i], self.offsets[i]) for i in range(self.config.n_layers)}
        assert len(st) == 1, "device-state decode needs every layer at the same position"
        s, n, o = st.pop()
        self._check_window(s, n)
        self.dev.copy_(torch.tensor([s, n, o, 0], dtype=torch.int64))

    def commit_device(self, layer_ind, L):
        """host bookkeeping of a device-state decode step that wrote L new rows behind the window
        (the device vector is refreshed once per forward, sync_device_state)"""
        assert self.start[layer_ind] + self.len[layer_ind] + L <= self.bufs[layer_ind][0].shape[1], \
            "cache capacity exceeded (enable_device_state(capacity))"
        self.len[layer_ind] += L
        self.offsets[layer_ind] += L

    def enable_cache_updates(self):
        self.should_update = True

    def disable_cache_updates(self):
        self.should_update = False

    def to(self, device="cuda", dtype=torch.bfloat16):
        self.device, self.dtype = device, dtype
        return self

    def reset(self, batch_size=1):
        self.batch_size = batch_size
        self.dev = None
        self.bufs = [None] * self.config.n_layers
        self.offsets = [0] * self.config.n_layers
        self.start = [0] * self.config.n_layers
        self.len = [0] * self.config.n_layers

    def rewind(self):
        """reset() that keeps every layer's buffers: an empty cache at the same addresses (the causal
        window samplers refill it for every generated frame; a captured HIP graph replays on it)."""
        assert self.bufs is not None, "Must reset cache before using"
        self.dev = None
        self.offsets = [0] * self.config.n_layers
        self.start = [0] * self.config.n_layers
        self.len = [0] * self.config.n_layers

    def _views(self, i, n):
        kb, vb = self.bufs[i]
        s = self.start[i]
        return kb[:, s:s + n], vb[:, s:s + n]

    def _reserve(self, i, need, like):
        """Room for `need` tokens from `start`: compact to 0 or grow (x2), keeping the live window."""
        buf = self.bufs[i]
        if buf is not None and self.start[i] + need <= buf[0].shape[1]:
            return
        n = self.len[i]
        cap = buf[0].shape[1] if buf is not None else 0
        if buf is None or need > cap:
            cap = max(2 * need, need + 16 * self.config.tokens_per_frame)
        new = tuple(torch.empty(like.shape[0], cap, like.shape[2], device=like.device, dtype=like.dtype)
                    for _ in range(2))
        if buf is not None and n:
            for dst, src in zip(new, self._views(i, n)):
                dst[:, :n].copy_(src)
        self.bufs[i], self.start[i] = new, 0

    @property
    def cache(self):
        assert self.bufs is not None, "Must reset cache before using"
        return [self._views(i, self.len[i]) if self.bufs[i] is not None else (None, None)
                for i in range(self.config.n_layers)]

    def get(self, layer_ind):
        assert self.bufs is not None, "Must reset cache before using"
        k, v = self._views(layer_ind, self.len[layer_ind])
        if self.noise_caches > 0.0:
            k = k + torch.randn_like(k) * self.noise_caches
            v = v + torch.randn_like(v) * self.noise_caches
        return k, v

    def extend_slots(self, layer_ind, L, like):
        """Views of the [B, L, d] slots behind the layer's cached window where the new frame's K/V go
        (written there directly by the decode rope kernel); ``extended(layer_ind, L)`` then gives
        [cache | new]."""
        assert self.noise_caches == 0.0, "the slots are read as stored (noise_caches must be 0)"
        n = self.len[layer_ind]
        self._reserve(layer_ind, n + L, like)
        kb, vb = self.bufs[layer_ind]
        s = self.start[layer_ind]
        return kb[:, s + n:s + n + L], vb[:, s + n:s + n + L]

    def extended(self, layer_ind, L):
        return self._views(layer_ind, self.len[layer_ind] + L)

    def extend(self, layer_ind, new_k, new_v):
        """[cache | new] as views of the layer's buffer (new K/V written once behind the cache)."""
        assert self.noise_caches == 0.0, "extend reads the cache as stored (noise_caches must be 0)"
        n, L = self.len[layer_ind], new_k.shape[1]
        self._reserve(layer_ind, n + L, new_k)
        self._write_behind(layer_ind, n, new_k, new_v)
        return self._views(layer_ind, n + L)

    def _write_behind(self, i, n, new_k, new_v):
        """new K/V into the rows behind the first n rows of layer i's window"""
        kb, vb = self.bufs[i]
        s, L = self.start[i], new_k.shape[1]
        kb[:, s + n:s + n + L].copy_(new_k)
        vb[:, s + n:s + n + L].copy_(new_v)

    def update(self, new_k, new_v, layer_ind):
        """kv_cache.py:47-58: the layer's cache becomes (new_k, new_v); a view returned by extend is
        committed in place."""
        assert self.bufs is not None, "Must reset cache before using"
        L = new_k.shape[1]
        self.offsets[layer_ind] += L - self.len[layer_ind]
        buf = self.bufs[layer_ind]
        if buf is not None and new_k.data_ptr() == buf[0][:, self.start[layer_ind]].data_ptr() \
                and new_k.stride() == buf[0].stride():
            self.len[layer_ind] = L
            return
        self.len[layer_ind] = 0
        self._reserve(layer_ind, L, new_k)
        kb, vb = self.bufs[layer_ind]
        kb[:, :L].copy_(new_k)
        vb[:, :L].copy_(new_v)
        self.start[layer_ind], self.len[layer_ind] = 0, L

    def truncate(self, truncate_amt, front=False):
        """kv_cache.py:60-75: eject ``truncate_amt`` FRAMES; front=True drops the newest tokens,
        front=False the oldest (the reference's naming, kept as is); offsets are unchanged."""
        amt = truncate_amt * self.config.tokens_per_frame
        for i in range(self.config.n_layers):
            amt_i = min(amt, self.len[i])
            if not front:
                self.start[i] = self._advanced(self.start[i], amt_i)
            self.len[i] -= amt_i
        self.sync_device_state()

    def _advanced(self, start, amt):
        """the window's start after the oldest `amt` rows are dropped"""
        return start + amt

    def length_at(self, idx):
        return self.len[idx]

    def get_offset(self, idx=0):
        return self.offsets[idx]

    def __len__(self):
        assert self.bufs is not None, "Must reset cache before using"
        return self.len[0]

    def n_frames(self):
        assert len(self) % self.config.tokens_per_frame == 0
        return len(self) // self.config.tokens_per_frame

    def clone(self):
        for i in range(self.config.n_layers):
            if self.bufs[i] is not None:
                self.bufs[i] = tuple(b.clone() for b in self.bufs[i])
        return self

    def detach(self):
        return self

    @property
    def shape(self):
        return self.cache[0][0].shape


class RingKVCache(SingleKVCache):
    """Endless decode (sampling/stream.py FrameStream; the reference's inference/causvid_pipeline.py):
    per layer a K/V ring ``[B, capacity, d]`` allocated once.  Logical row i of the live window lives at
    physical row ``(start + i) % capacity``; writes behind the window and ``truncate(k, front=False)``
    wrap, so neither the addresses nor the size ever change, however many frames pass through (a
    captured HIP graph stays valid across wraps).  The decode kernels' ring forms follow the device
    state vector {start, cached tokens, rope offset} (``owlk_qk_rope_fwd_kv_ring``,
    ``owlk_attn_decode_ring_fwd``); ``rebase`` re-rotates the cached K to smaller RoPE positions
    (``owlk_rope_rebase``), so the positions never leave the table either.

    A wrapped window has no view: ``get`` / ``cache`` / ``extend`` return gathered copies."""

    ring = True

    def __init__(self, config, capacity, rope=None):
        super().__init__(config)
        assert capacity > 0
        self.capacity = int(capacity)
        self.rope = rope  # the model's RoPE table module (cos / sin), for rebase

    def _alloc(self, i, like):
        if self.bufs[i] is None:
            self.bufs[i] = tuple(torch.empty(like.shape[0], self.capacity, like.shape[2], device=like.device,
                                             dtype=like.dtype) for _ in range(2))

    def _rows(self, i, first, n):
        """physical rows of the logical rows first .. first + n - 1 of layer i's window"""
        dev = self.bufs[i][0].device
        return (torch.arange(first, first + n, device=dev) + self.start[i]) % self.capacity

    def _views(self, i, n):
        kb, vb = self.bufs[i]
        idx = self._rows(i, 0, n)
        return kb.index_select(1, idx), vb.index_select(1, idx)

    def _reserve(self, i, need, like):
        assert need <= self.capacity, f"ring capacity exceeded ({need} > {self.capacity} rows)"
        self._alloc(i, like)

    def enable_device_state(self, capacity=None):
        """The position on the device (the ring decode kernels read it); the buffers already have their
        final size, so this only creates the state vector."""
        assert capacity is None or capacity <= self.capacity, "a ring cache does not grow"
        assert all(b is not None for b in self.bufs), "enable_device_state after the context pass"
        self._create_device_state()

    def _check_window(self, s, n):
        assert 0 <= s < self.capacity and 0 <= n <= self.capacity

    def commit_device(self, layer_ind, L):
        assert self.len[layer_ind] + L <= self.capacity, "ring capacity exceeded (evict before committing)"
        self.len[layer_ind] += L
        self.offsets[layer_ind] += L

    def advance(self, L, max_rows, device=True):
        """A streamed frame of L rows, already written behind the window by the frame's last forward, is
        committed and the oldest L rows are evicted once more than max_rows are cached:

            len += L; offsets += L;  then, if len > max_rows:  start = (start + L) % capacity; len -= L

        -- commit_device on every layer, then truncate(1, front=False) when over, as one rule.  It is
        applied to the host mirror of every layer; with device=True the device vector follows by one
        ``owlk_ring_advance`` launch (no host-to-device copy, so a captured frame holds it).  Under graph
        capture only the launch is recorded: a capture executes nothing, so the mirror stays (the caller
        advances it once per replay with device=False)."""
        L, max_rows = int(L), int(max_rows)
        assert L > 0 and 0 < max_rows and max_rows + L <= self.capacity, \
            f"advance: need 0 < L, 0 < max_rows and max_rows + L <= capacity ({L}, {max_rows}, {self.capacity})"
        if device:
            from .. import kernels as K
            assert self.dev is not None, "advance(device=True) after enable_device_state()"
            K.ring_advance(self.dev, L, max_rows, self.capacity)
            if torch.cuda.is_current_stream_capturing():
                return
        for i in range(self.config.n_layers):
            assert self.len[i] + L <= self.capacity, "ring capacity exceeded (evict before committing)"
            self.len[i] += L
            self.offsets[i] += L
            if self.len[i] > max_rows:
                self.start[i] = (self.start[i] + L) % self.capacity
                self.len[i] -= L

    def device_state(self):
        """(start, cached, offset) read back from the device vector (a synchronising copy): for tests and
        for a stream's close(), which compares it with the host mirror."""
        assert self.dev is not None, "device_state after enable_device_state()"
        s, n, o, _ = self.dev.tolist()
        return s, n, o

    def extend_slots(self, layer_ind, L, like):
        raise RuntimeError("RingKVCache: the new rows may wrap, so there is no slot view; the ring rope kernel "
                           "(kernels.qk_rope_fwd_kv_ring) writes them")

    def _write_behind(self, i, n, new_k, new_v):
        """wrapping (extend then returns [cache | new] as gathered copies)"""
        kb, vb = self.bufs[i]
        idx = self._rows(i, n, new_k.shape[1])
        kb.index_copy_(1, idx, new_k)
        vb.index_copy_(1, idx, new_v)

    def update(self, new_k, new_v, layer_ind):
        """the layer's cache becomes (new_k, new_v), from row 0 (the context pass fills the ring)"""
        assert self.bufs is not None, "Must reset cache before using"
        L = new_k.shape[1]
        assert L <= self.capacity, f"ring capacity exceeded ({L} > {self.capacity} rows)"
        self._alloc(layer_ind, new_k)
        self.offsets[layer_ind] += L - self.len[layer_ind]
        kb, vb = self.bufs[layer_ind]
        kb[:, :L].copy_(new_k)
        vb[:, :L].copy_(new_v)
        self.start[layer_ind], self.len[layer_ind] = 0, L

    def _advanced(self, start, amt):
        return (start + amt) % self.capacity

    def rebase(self, shift_tokens, rope=None):
        """Lower every live key's RoPE position by `shift_tokens` (whole frames): each layer's cached K is
        re-rotated in place (V carries no position), then the offsets drop.  Valid for tables whose
        angles are linear in the frame index: MotionRoPE, Audio1DRoPE, and OrthoRoPE, whose time axis
        alone moves with the frame (angle a_r + f * delta).  The rotation is formed from two rows of the
        table in hand, so the table need not be a prefix of a longer one (OrthoRoPE's is not).  Which
        stream may rebase which table is the stream classes' choice (sampling/stream.py rebase_ropes)."""
        from .. import kernels as K
        rope = rope if rope is not None else self.rope
        assert rope is not None, "rebase needs the model's RoPE tables"
        tpf = self.config.tokens_per_frame
        assert shift_tokens >= 0 and shift_tokens % tpf == 0, "rebase by whole frames"
        if shift_tokens == 0:
            return
        H = self.config.n_heads
        D = self.config.d_model // H
        for i in range(self.config.n_layers):
            old = self.offsets[i] - self.len[i]
            if old < shift_tokens:
                raise RuntimeError(f"rebase by {shift_tokens} tokens would move the oldest cached key (position "
                                   f"{old}) below 0")
            if self.len[i]:
                K.rope_rebase(self.bufs[i][0], H, D, self.start[i], self.len[i], rope.cos, rope.sin, old,
                              old - shift_tokens)
            self.offsets[i] -= shift_tokens
        self.sync_device_state()

    def clone(self):
        raise RuntimeError("RingKVCache keeps fixed buffers; clone is not supported")


class SlotRingKVCache:
    """Many sessions in one batch (sampling/stream_pool.py StreamPool): per layer K/V rings
    ``[batch_rows, capacity, d]`` allocated once, ``batch_rows`` = n_slots, or 2 n_slots with CFG
    ([cond | uncond]: batch row b belongs to slot ``b % n_slots``), and ONE device state ``[n_slots, 4]``, row s
    = {start, cached tokens, rope offset, live}, which the slot forms of the ring kernels read
    (``owlk_qk_rope_fwd_kv_ring_slots``, ``owlk_attn_decode_ring_slots_fwd``) and ``owlk_ring_advance_slots``
    moves.  Every layer of a slot advances together, so the host keeps one exact mirror per slot (start, len,
    offsets, live).  Decode only: a slot's context is cached through ``slot_view`` (a RingKVCache over that
    slot's batch rows), a streamed frame is committed by ``advance``; idle slots cost no cache traffic."""

    ring = True
    should_update = False  # frames are committed by advance(), not by the forward's bookkeeping
    noise_caches = 0.0

    def __init__(self, config, capacity, n_slots, batch_rows, rope=None, device="cuda", dtype=torch.bfloat16):
        assert capacity > 0 and n_slots > 0 and batch_rows in (n_slots, 2 * n_slots)
        self.config = config
        self.capacity = int(capacity)
        self.n_slots = int(n_slots)
        self.rope = rope
        d = config.d_model
        self.bufs = [tuple(torch.empty(batch_rows, self.capacity, d, device=device, dtype=dtype) for _ in range(2))
                     for _ in range(config.n_layers)]
        self.dev = torch.zeros(self.n_slots, 4, dtype=torch.int64, device=device)
        self.start = [0] * self.n_slots
        self.len = [0] * self.n_slots
        self.offsets = [0] * self.n_slots
        self.live = [False] * self.n_slots

    # ------------------------------------------------------------------ slots
    def free_slot(self):
        """the lowest idle slot, or None when every slot is live"""
        return next((s for s in range(self.n_slots) if not self.live[s]), None)

    def live_slots(self):
        return [s for s in range(self.n_slots) if self.live[s]]

    def slot_view(self, slot):
        """A RingKVCache over the slot's batch rows ``bufs[slot::n_slots]`` (strided views, nothing allocated)
        for that session's context pass: the forward's ``update`` writes rows 0.. of the slot's rings."""
        view = RingKVCache(self.config, self.capacity, rope=self.rope)
        view.reset(self.bufs[0][0].shape[0] // self.n_slots)
        view.bufs = [(kb[slot::self.n_slots], vb[slot::self.n_slots]) for kb, vb in self.bufs]
        return view

    def _sync_slot(self, slot):
        """the slot's mirror -> its device row (outside graph capture: a small host-to-device copy)"""
        s, n, o = self.start[slot], self.len[slot], self.offsets[slot]
        assert 0 <= s < self.capacity and 0 <= n <= self.capacity and o >= 0
        self.dev[slot].copy_(torch.tensor([s, n, o, int(self.live[slot])], dtype=torch.int64))

    def open_slot(self, slot, rows):
        """the slot goes live with `rows` context rows cached from physical row 0 at positions 0 .. rows - 1"""
        assert not self.live[slot], f"slot {slot} is live"
        assert 0 < rows <= self.capacity
        self.start[slot], self.len[slot], self.offsets[slot], self.live[slot] = 0, int(rows), int(rows), True
        self._sync_slot(slot)

    def close_slot(self, slot):
        """the slot goes idle on host and device; its rows stay where they are and are never read again (a
        later open_slot starts a new window)"""
        assert self.live[slot], f"slot {slot} is idle"
        self.start[slot], self.len[slot], self.offsets[slot], self.live[slot] = 0, 0, 0, False
        self._sync_slot(slot)

    # ------------------------------------------------------------------ what the DiT's cached forward reads
    def get_offset(self, idx=0):
        """the largest rope offset among the live slots (0 with none): the one an eager forward's table check
        has to hold for, since every live slot's offset is at most this"""
        return max((self.offsets[s] for s in self.live_slots()), default=0)

    def length_at(self, idx=0):
        return max((self.len[s] for s in self.live_slots()), default=0)

    def commit_device(self, layer_ind, L):
        raise RuntimeError("SlotRingKVCache: frames are committed by advance(), once for every layer and slot")

    def enable_cache_updates(self):
        raise RuntimeError("SlotRingKVCache: cache a slot's context through slot_view(slot)")

    def advance(self, L, max_rows, device=True):
        """RingKVCache.advance's rule on every live slot:

            len += L; offsets += L;  then, if len > max_rows:  start = (start + L) % capacity; len -= L

        device=True: one ``owlk_ring_advance_slots`` launch moves the device rows (under graph capture only
        the launch is recorded and the mirror stays; the caller advances it once per replay with
        device=False)."""
        L, max_rows = int(L), int(max_rows)
        assert L > 0 and 0 < max_rows and max_rows + L <= self.capacity, \
            f"advance: need 0 < L, 0 < max_rows and max_rows + L <= capacity ({L}, {max_rows}, {self.capacity})"
        if device:
            from .. import kernels as K
            K.ring_advance_slots(self.dev, L, max_rows, self.capacity)
            if torch.cuda.is_current_stream_capturing():
                return
        for s in self.live_slots():
            assert self.len[s] + L <= self.capacity, "ring capacity exceeded (evict before committing)"
            self.len[s] += L
            self.offsets[s] += L
            if self.len[s] > max_rows:
                self.start[s] = (self.start[s] + L) % self.capacity
                self.len[s] -= L

    def host_state(self):
        """the mirror as device_state() returns the device rows"""
        return [(self.start[s], self.len[s], self.offsets[s], int(self.live[s])) for s in range(self.n_slots)]

    def device_state(self):
        """every row (start, cached, offset, live) read back from the device (a synchronising copy)"""
        return [tuple(r) for r in self.dev.tolist()]

    def rebase(self, slot, shift_tokens, rope=None):
        """RingKVCache.rebase for one slot: its cached K rows (the slot's batch rows of every layer) are
        re-rotated in place to positions lower by `shift_tokens` (``owlk_rope_rebase`` with the slot view's
        batch stride), then its offset drops and its device row is rewritten.  Other slots are untouched."""
        from .. import kernels as K
        rope = rope if rope is not None else self.rope
        assert rope is not None, "rebase needs the model's RoPE tables"
        assert self.live[slot], f"slot {slot} is idle"
        tpf = self.config.tokens_per_frame
        assert shift_tokens >= 0 and shift_tokens % tpf == 0, "rebase by whole frames"
        if shift_tokens == 0:
            return
        H = self.config.n_heads
        D = self.config.d_model // H
        old = self.offsets[slot] - self.len[slot]
        if old < shift_tokens:
            raise RuntimeError(f"rebase by {shift_tokens} tokens would move slot {slot}'s oldest cached key (position "
                               f"{old}) below 0")
        if self.len[slot]:
            for kb, _ in self.bufs:
                K.rope_rebase(kb[slot::self.n_slots], H, D, self.start[slot], self.len[slot], rope.cos, rope.sin, old,
                              old - shift_tokens)
        self.offsets[slot] -= shift_tokens
        self._sync_slot(slot)
