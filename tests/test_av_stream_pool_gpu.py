"""Model-level tests of multi-session audio + video streaming (owl_wms/sampling/stream_pool.py: AVStreamPool on
the MMDiT, AVDiTStreamPool on the DiT backbone, on a SlotRingKVCache) on the tiny models of
tests/test_av_stream_gpu.py (mmdit) and tests/test_av_dit_stream_gpu.py (dit): d_model 128, 2 heads, 2 layers, 65
tokens per frame, local_window 2, global_window 4; n_steps 4, noise_prev 0.2, a 32-frame RoPE table unless stated.

Tolerances.  One slot against the B = 1 stream class, a session against itself with other neighbours / in another
slot / in a reused slot, and the three graph modes against each other: torch.equal on video and audio -- the same
kernels on the same rows at the same batch size, the same draws.  A session of a 3-slot pool against its own B = 1
stream: the decode GEMMs choose their plan by M, so equality is not expected; rel-L2 <= 2e-2, the project's bound
for sampled latents between equivalent decode paths (tests/test_av_stream_gpu.py).  A rebased session against the
same pool on a table long enough not to rebase: the same bound, as the streams' rebase tests.

Measured on an MI355X (rel-L2, video / audio; the tests print them, DESIGN.md "Multi-session audio + video
streaming" records them): sessions A / B / C of the joined pool against their B = 1 streams 0 / 0 on both
backbones; the rebased sessions A and X against a 32-frame table: mmdit motion 5.0e-4 / 7.5e-5 and 4.1e-4 / 1.6e-4,
dit motion 4.7e-4 / 1.5e-4 and 5.1e-4 / 9.0e-4, dit ortho 4.1e-4 / 6.0e-4 and 4.3e-4 / 2.0e-5."""
import functools

import pytest
import torch

import test_av_dit_stream_gpu as DT
import test_av_stream_gpu as MM
from test_av_stream_gpu import _inputs, rel

pytestmark = pytest.mark.gpu

KW = dict(n_steps=4, noise_prev=0.2)
MODES = (False, True, "frame")
BACKBONES = ("mmdit", "dit")
TPF = 65


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _model(backbone, n_frames=32, rope_impl="motion", copy=0):
    return MM._model(n_frames, rope_impl) if backbone == "mmdit" else DT._model(n_frames, rope_impl, copy)


def _session(data_seed, init, ticks, seed):
    """one session: (context video [1, init, ...], audio [1, init, 16], mouse / btn for init + ticks frames, seed)"""
    return (*_inputs(1, init, init + ticks, seed=data_seed), seed)


SESSIONS = {}  # filled on first use (the inputs live on the GPU)


def sessions():
    if not SESSIONS:
        SESSIONS.update(A=_session(7, 3, 12, 321), B=_session(8, 2, 12, 654), C=_session(9, 1, 12, 987),
                        D=_session(10, 2, 12, 111), X=_session(11, 4, 12, 222))
    return SESSIONS


def run_pool(core, n_slots, script, ticks, **kw):
    """Drive the core's pool class: script {tick: [("open", name) | ("close", name), ...]} applied before that
    tick.  -> ({name: (video [1, n, c, h, w], audio [1, n, ca])}, info) with info: slot per name, the ticks at
    which each name's slot rebased, the host state rows before close, the pool (closed, its state check passed),
    buffer addresses and shapes at construction and at the end."""
    from owl_wms.sampling.stream_pool import av_pool_cls
    ses = sessions()
    frames, slot_of, age, rebased, slots = {}, {}, {}, {}, {}

    def bufs(pool):
        c = pool.kv_cache
        return [(kb.data_ptr(), vb.data_ptr(), tuple(kb.shape), tuple(vb.shape)) for kb, vb in c.bufs] + \
            [(c.dev.data_ptr(), tuple(c.dev.shape))]

    with av_pool_cls(core.config.backbone)(core, n_slots, **KW, **kw) as pool:
        bufs0 = bufs(pool)
        for tick in range(ticks):
            for act, name in script.get(tick, ()):
                if act == "open":
                    slots[name] = slot_of[name] = pool.open(*ses[name])
                    age[name], frames[name], rebased[name] = 0, [], []
                else:
                    pool.close_slot(slot_of.pop(name))
            ctrl = {}
            for name, slot in slot_of.items():
                x, _, mouse, btn, _ = ses[name]
                i = x.size(1) + age[name]
                ctrl[slot] = (mouse[:, i:i + 1], btn[:, i:i + 1])
            before = list(pool.rebases)
            out = pool.step(ctrl)
            assert sorted(out) == sorted(ctrl)
            for name, slot in slot_of.items():
                v, a = out[slot]
                assert v.shape == (1, 1, 32, 8, 8) and a.shape == (1, 1, 16)
                frames[name].append((v, a))
                age[name] += 1
                if pool.rebases[slot] > before[slot]:
                    rebased[name].append(tick)
        state = pool.kv_cache.host_state()
        assert pool.kv_cache.device_state() == state  # the device rows equal the host mirror (close() checks again)
        bufs1 = bufs(pool)
    torch.cuda.synchronize()
    info = dict(slots=slots, rebased=rebased, state=state, pool=pool, bufs0=bufs0, bufs1=bufs1)
    return {n: (torch.cat([v for v, _ in f], 1), torch.cat([a for _, a in f], 1)) for n, f in frames.items()}, info


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def finite(*pairs):
    return all(bool(torch.isfinite(t.float()).all()) for p in pairs for t in p)


def _draw_shapes(x, audio):
    """a B = 1 audio + video stream's draws, in order: context video, context audio, then per frame video noise,
    audio noise, video re-noise, audio re-noise"""
    one = [(1, 1, *x.shape[2:]), (1, 1, audio.shape[2])]
    return [tuple(x.shape), tuple(audio.shape)] + one + one


def _generator_matches_default(seed, shapes):
    """a fresh device generator seeded `seed` draws what the default generator draws after manual_seed(seed)"""
    torch.manual_seed(seed)
    a = [torch.randn(s, device="cuda", dtype=torch.bfloat16) for s in shapes]
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    b = [torch.randn(s, generator=g, device="cuda", dtype=torch.bfloat16) for s in shapes]
    return all(torch.equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def single_stream(backbone, name, frames, cfg_scale, max_cached_frames, n_frames=32):
    """the session alone on the backbone's B = 1 stream class (eager; its graph modes give the same bits,
    tests/test_av_stream_gpu.py, tests/test_av_dit_stream_gpu.py, tests/test_frame_graph_gpu.py)"""
    from owl_wms.sampling.stream import av_stream_cls
    x, audio, mouse, btn, seed = sessions()[name]
    init = x.size(1)
    assert _generator_matches_default(seed, _draw_shapes(x, audio))
    torch.manual_seed(seed)
    with av_stream_cls(backbone)(_model(backbone, n_frames).core, cfg_scale=cfg_scale,
                                 max_cached_frames=max_cached_frames, **KW) as s:
        s.start(x, audio, mouse, btn)
        out = [s.step(mouse[:, init + i:init + i + 1], btn[:, init + i:init + i + 1]) for i in range(frames)]
    return torch.cat([o[0] for o in out], 1), torch.cat([o[1] for o in out], 1)


def test_session_generator_reproduces_the_default_generator():
    """the premise of the comparisons with the B = 1 streams, on plain randn calls of the streams' shapes"""
    x, audio, *_ = sessions()["A"]
    shapes = _draw_shapes(x, audio)
    assert shapes[:4] == [(1, 3, 32, 8, 8), (1, 3, 16), (1, 1, 32, 8, 8), (1, 1, 16)]
    assert _generator_matches_default(321, shapes + shapes[2:])


@pytest.mark.parametrize("graphed", MODES)
@pytest.mark.parametrize("cfg_scale", [1.3, 1.0])
@pytest.mark.parametrize("backbone", BACKBONES)
def test_one_slot_is_the_single_stream(backbone, cfg_scale, graphed):
    """n_slots 1, 3 context frames, max_cached_frames 4, 10 frames (the 5-frame ring wraps twice): the bits of
    the B = 1 stream class with the same seed, video and audio."""
    ref = single_stream(backbone, "A", 10, cfg_scale, 4)
    out, info = run_pool(_model(backbone).core, 1, {0: [("open", "A")]}, 10, cfg_scale=cfg_scale,
                         max_cached_frames=4, graphed=graphed)
    assert out["A"][0].shape == ref[0].shape == (1, 10, 32, 8, 8) and out["A"][1].shape == ref[1].shape == (1, 10, 16)
    assert finite(ref)
    assert torch.equal(out["A"][0], ref[0]) and torch.equal(out["A"][1], ref[1])
    pool = info["pool"]
    assert pool.frames_generated == [10] and pool.rebases == [0] and pool.ticks == 10
    assert info["state"] == [((9 * TPF) % (5 * TPF), 4 * TPF, 13 * TPF, 1)]  # 9 evictions on a 5-frame ring
    assert pool.graph_replays == {False: 0, True: 10 * 4 - 1, "frame": 9}[graphed]
    assert pool.kv_cache.bufs[0][0].shape == (2 if cfg_scale != 1.0 else 1, 5 * TPF, 128)


ALONE = {0: [("open", "A")]}
JOINED = {0: [("open", "A")], 3: [("open", "B")], 6: [("open", "C")]}  # B after tick 2, C after tick 5
SECOND = {0: [("open", "X"), ("open", "A")], 4: [("close", "X")]}  # A in slot 1, slot 0 closed half-way


@functools.lru_cache(maxsize=None)
def three_slots(backbone, setting, graphed, max_cached_frames=4, n_frames=32, ticks=8):
    script = {"alone": ALONE, "joined": JOINED, "second": SECOND}[setting]
    return run_pool(_model(backbone, n_frames).core, 3, script, ticks, cfg_scale=1.3,
                    max_cached_frames=max_cached_frames, graphed=graphed)


@pytest.mark.parametrize("backbone", BACKBONES)
def test_neighbours_and_slot_number_do_not_matter(backbone):
    """Session A alone in slot 0, in slot 0 with B and C joining after ticks 2 and 5, and in slot 1 beside a
    session that leaves half-way: its 8 frames bit for bit the same, in all three graph modes; the device state
    rows equal the host mirror at close() in every run (run_pool, and close() itself)."""
    ref, _ = three_slots(backbone, "alone", False)
    assert ref["A"][0].shape == (1, 8, 32, 8, 8) and ref["A"][1].shape == (1, 8, 16)
    for setting in ("alone", "joined", "second"):
        for graphed in MODES:
            out, info = three_slots(backbone, setting, graphed)
            assert info["slots"]["A"] == (1 if setting == "second" else 0)
            assert same(out["A"], ref["A"]), (setting, graphed)
            assert finite(*out.values()), (setting, graphed)
    out, info = three_slots(backbone, "joined", "frame")
    assert info["slots"] == {"A": 0, "B": 1, "C": 2}
    assert [out[n][0].shape[1] for n in "ABC"] == [8, 5, 2]
    a, b, c = info["state"]
    # A: 3 + 8 frames through a 5-frame ring (7 evictions); B: 2 + 5 (3 evictions); C: 1 + 2, nothing evicted
    assert a == ((7 * TPF) % (5 * TPF), 4 * TPF, 11 * TPF, 1) and b == (3 * TPF, 4 * TPF, 7 * TPF, 1)
    assert c == (0, 3 * TPF, 3 * TPF, 1)
    _, info = three_slots(backbone, "second", "frame")
    assert info["state"][0] == (0, 0, 0, 0) and info["state"][1][3] == 1  # the closed slot is idle on both sides


@pytest.mark.parametrize("backbone", BACKBONES)
def test_sessions_match_their_single_streams(backbone):
    """Each session of the joined pool against its own B = 1 stream, same seed and controls: rel-L2 <= 2e-2 on
    video and on audio (the GEMMs' plan follows M, so no equality)."""
    out, _ = three_slots(backbone, "joined", False)
    for name in "ABC":
        n = out[name][0].shape[1]
        ref = single_stream(backbone, name, n, 1.3, 4)
        rv, ra = rel(out[name][0], ref[0]), rel(out[name][1], ref[1])
        print(f"{backbone} pool session {name} vs its B = 1 stream, {n} frames: video rel-L2 {rv:.3e}, audio rel-L2 "
              f"{ra:.3e}")
        assert rv <= 2e-2, (name, rv)
        assert ra <= 2e-2, (name, ra)


@pytest.mark.parametrize("backbone", BACKBONES)
def test_slot_reuse_leaks_nothing(backbone):
    """A leaves after tick 4 and D takes its slot beside B: D's frames are those of D in a fresh pool in the
    same slot beside a live slot 1; rings and state keep their addresses and sizes since construction."""
    core = _model(backbone).core
    reuse = {0: [("open", "A"), ("open", "B")], 5: [("close", "A"), ("open", "D")]}
    fresh = {0: [("open", "D"), ("open", "B")]}
    for graphed in MODES:
        out, info = run_pool(core, 3, reuse, 9, cfg_scale=1.3, max_cached_frames=4, graphed=graphed)
        assert info["slots"] == {"A": 0, "B": 1, "D": 0} and out["D"][0].shape[1] == 4 and out["A"][0].shape[1] == 5
        want, winfo = run_pool(core, 3, fresh, 4, cfg_scale=1.3, max_cached_frames=4, graphed=graphed)
        assert winfo["slots"] == {"D": 0, "B": 1}
        assert same(out["D"], want["D"]), graphed
        assert info["bufs0"] == info["bufs1"] and len(info["bufs0"]) == 2 + 1
        assert all(b[2] == (6, 5 * TPF, 128) for b in info["bufs0"][:2]) and info["bufs0"][2][1] == (3, 4)
        assert info["pool"].frames_generated[0] == 4  # the slot's counter restarted with D


def _ortho_long():
    """a 32-frame dit model with the weights of the 8-frame ortho one whose tables carry the 8-frame OrthoRoPE law
    extended to 32 frames (angles a_r + f * delta in fp64, as tests/test_av_dit_stream_gpu.py builds its
    reference: the 32-frame OrthoRoPE table itself is another law)"""
    short, long_ = _model("dit", 8, "ortho"), _model("dit", 32, "ortho", copy=2)
    rs, rl = short.core.transformer.rope, long_.core.transformer.rope
    ang = rs.get_freqs(short.core.config).double().view(8, TPF, -1)
    delta = (ang[7] - ang[0]) / 7.0
    ext = ang[0][None] + torch.arange(32, dtype=torch.float64)[:, None, None] * delta[None]
    rl.cos.copy_(ext.cos().float().view(32 * TPF, -1))
    rl.sin.copy_(ext.sin().float().view(32 * TPF, -1))
    return long_


@pytest.mark.parametrize("backbone,rope_impl", [("mmdit", "motion"), ("dit", "motion"), ("dit", "ortho")])
def test_slots_rebase_on_their_own(backbone, rope_impl):
    """8-frame table, max_cached_frames 4, A from tick 0 and X from tick 2 (3 and 4 context frames), 12 ticks:
    each slot rebases when ITS positions reach the table's end, at different ticks; the three modes agree bit
    for bit; each session within rel-L2 2e-2 of the same pool on a 32-frame table, which never rebases."""
    script = {0: [("open", "A")], 2: [("open", "X")]}
    short = _model(backbone, 8, rope_impl)
    long_ = _ortho_long() if rope_impl == "ortho" else _model(backbone, 32, rope_impl)
    for (ka, a_), (kb_, b_) in zip(sorted(short.state_dict().items()), sorted(long_.state_dict().items())):
        assert ka == kb_ and torch.equal(a_, b_), ka
    runs = {g: run_pool(short.core, 3, script, 12, cfg_scale=1.3, max_cached_frames=4, graphed=g) for g in MODES}
    out, info = runs[False]
    # frames of offset before tick t: A 3 + t, X 4 + (t - 2); a slot rebases (to 4 cached frames) at offset 8
    assert info["rebased"] == {"A": [5, 9], "X": [6, 10]}
    assert info["pool"].rebases[:2] == [2, 2]
    for g in MODES[1:]:
        assert runs[g][1]["rebased"] == info["rebased"]
        for name in "AX":
            assert same(runs[g][0][name], out[name]), (g, name)
    ref, rinfo = run_pool(long_.core, 3, script, 12, cfg_scale=1.3, max_cached_frames=4, graphed=False)
    assert rinfo["rebased"] == {"A": [], "X": []}
    for name in "AX":
        rv, ra = rel(out[name][0], ref[name][0]), rel(out[name][1], ref[name][1])
        print(f"rebased {backbone} / {rope_impl} pool session {name} vs a 32-frame table: video rel-L2 {rv:.3e}, "
              f"audio rel-L2 {ra:.3e}")
        assert finite(out[name])
        assert rv <= 2e-2, (name, rv)
        assert ra <= 2e-2, (name, ra)


def test_mmdit_pool_refuses_ortho_at_the_end_of_its_table():
    """the MMDiT pool streams OrthoRoPE to the end of its table, then raises the stream's message"""
    from owl_wms.sampling.stream_pool import AVStreamPool
    x, audio, mouse, btn, seed = sessions()["A"]
    with AVStreamPool(_model("mmdit", 8, "ortho").core, 2, n_steps=2, cfg_scale=1.0, max_cached_frames=4) as pool:
        s = pool.open(x, audio, mouse, btn, seed)
        for i in range(5):  # positions 3..7: inside the table
            v, a = pool.step({s: (mouse[:, 3 + i:4 + i], btn[:, 3 + i:4 + i])})[s]
            assert finite((v, a))
        with pytest.raises(RuntimeError, match="cannot be rebased by this stream"):
            pool.step({s: (mouse[:, 8:9], btn[:, 8:9])})
        assert pool.frames_generated[s] == 5 and pool.rebases[s] == 0
    torch.cuda.synchronize()


def test_attn_takes_a_65_row_frame_on_a_slot_cache():
    """Attn._attend with a SlotRingKVCache and a 65-row frame at head_dim 64 (a RuntimeError before the wide slot
    form): the wide slot pair, finite rows for the live slot, zero rows for the idle one; 81 rows still refuse."""
    from owl_wms.nn.attn import Attn
    from owl_wms.nn.kv_cache import SlotRingKVCache
    core = _model("dit").core
    attn = next(m for m in core.transformer.modules() if isinstance(m, Attn))
    cache = SlotRingKVCache(core.config, 5 * TPF, 2, 2, rope=core.transformer.rope)
    for kb, vb in cache.bufs:
        kb.normal_(), vb.normal_()
    cache.open_slot(0, 2 * TPF)
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(2 * TPF, 3 * 128, generator=g).bfloat16().cuda()
    o = attn._attend(qkv, 2, TPF, None, cache)
    assert o.shape == (2, TPF, 128) and torch.isfinite(o[0].float()).all() and (o[1] == 0).all()
    assert cache.host_state() == [(0, 2 * TPF, 2 * TPF, 1), (0, 0, 0, 0)] == cache.device_state()
    with pytest.raises(RuntimeError, match="at most 80 rows"):
        attn._attend(torch.zeros(2 * 81, 3 * 128, device="cuda", dtype=torch.bfloat16), 2, 81, None, cache)


@pytest.mark.parametrize("backbone", BACKBONES)
def test_pool_errors(backbone):
    from owl_wms.sampling.stream_pool import av_pool_cls
    core = _model(backbone).core
    ses = sessions()
    with av_pool_cls(backbone)(core, 2, cfg_scale=1.3, max_cached_frames=3, **KW) as pool:
        assert pool.step({}) == {} and pool.live == []
        with pytest.raises(ValueError, match="context frames"):
            pool.open(*ses["X"])  # 4 context frames, max_cached_frames 3
        x, audio, mouse, btn, seed = ses["A"]
        with pytest.raises(ValueError, match="context video"):
            pool.open(x, audio[:, :2], mouse, btn, seed)
        a = pool.open(*ses["A"])
        assert a == 0 and pool.live == [0]
        c = (mouse[:, 3:4], btn[:, 3:4])
        with pytest.raises(ValueError, match="live slots"):
            pool.step({})  # the live slot's controls are missing
        with pytest.raises(ValueError, match="live slots"):
            pool.step({0: c, 1: c})  # an idle slot's controls
        with pytest.raises(ValueError, match="not live"):
            pool.close_slot(1)
        with pytest.raises(RuntimeError, match="open"):
            pool.start(x, audio, mouse, btn)
        assert pool.open(*ses["B"]) == 1
        with pytest.raises(RuntimeError, match="slots are live"):
            pool.open(*ses["C"])
        out = pool.step({0: c, 1: (ses["B"][2][:, 2:3], ses["B"][3][:, 2:3])})
        assert sorted(out) == [0, 1] and finite(*out.values())
        pool.close_slot(0)
        assert pool.open(*ses["C"]) == 0  # the lowest free slot again
