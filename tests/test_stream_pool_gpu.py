"""Model-level tests of multi-session streaming (owl_wms/sampling/stream_pool.py: StreamPool on a
SlotRingKVCache) on the tiny GameRFT of tests/test_stream_gpu.py: 2 layers, 2 heads, d_model 128 / 256 (head_dim
64 / 128), 64 tokens per frame, MotionRoPE; n_steps 4, noise_prev 0.2, a 32-frame RoPE table unless stated.

Tolerances.  One slot against FrameStream, a session against itself with other neighbours / in another slot /
in a reused slot, and the three graph modes against each other: torch.equal -- the same kernels on the same
rows at the same batch size, the same draws.  A session of a 3-slot pool against its own B = 1 FrameStream: the
decode GEMMs choose their split-K plan by M, so equality is not expected; rel-L2 <= 2e-2, the project's bound
for sampled latents between equivalent decode paths (tests/test_stream_gpu.py).  A rebased session against the
same pool on a table long enough not to rebase: the same bound, as FrameStream's rebase test.

Measured on an MI355X (rel-L2; the tests print them, DESIGN.md §4 "Multi-session streaming" records them):
sessions A / B / C of the joined pool against their FrameStreams 0 / 0 / 0 at d_model 128 and 8.5e-4 / 0 / 4.1e-4
at 256; the rebased sessions against a 32-frame table 4.5e-4 / 4.7e-4 at d_model 128 and 9.2e-4 / 8.8e-4 at 256."""
import functools

import pytest
import torch

from test_stream_gpu import _inputs, _model, rel

pytestmark = pytest.mark.gpu

KW = dict(n_steps=4, noise_prev=0.2)
MODES = (False, True, "frame")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _session(data_seed, init, ticks, seed):
    """one session: (context x [1, init, ...], mouse / btn for init + ticks frames, noise seed)"""
    x, mouse, btn = _inputs(1, init, init + ticks, seed=data_seed)
    return x, mouse, btn, seed


SESSIONS = {}  # filled on first use (the inputs live on the GPU)


def sessions():
    if not SESSIONS:
        SESSIONS.update(A=_session(7, 3, 14, 321), B=_session(8, 2, 14, 654), C=_session(9, 1, 14, 987),
                        D=_session(10, 2, 14, 111), X=_session(11, 4, 14, 222))
    return SESSIONS


def run_pool(core, n_slots, script, ticks, **kw):
    """Drive a StreamPool: script {tick: [("open", name) | ("close", name), ...]} applied before that tick.
    -> (frames {name: [1, n, c, h, w]}, info) with info: slot per name, the ticks at which each name's slot
    rebased, the host state rows before close, the pool (closed, its state check passed), buffer addresses
    and row counts at construction and at the end."""
    from owl_wms.sampling.stream_pool import StreamPool
    ses = sessions()
    frames, slot_of, age, rebased, slots = {}, {}, {}, {}, {}

    def bufs(pool):
        c = pool.kv_cache
        return [(kb.data_ptr(), vb.data_ptr(), tuple(kb.shape), tuple(vb.shape)) for kb, vb in c.bufs] + \
            [(c.dev.data_ptr(), tuple(c.dev.shape))]

    with StreamPool(core, n_slots, **KW, **kw) as pool:
        bufs0 = bufs(pool)
        for tick in range(ticks):
            for act, name in script.get(tick, ()):
                if act == "open":
                    x, mouse, btn, seed = ses[name]
                    slots[name] = slot_of[name] = pool.open(x, mouse, btn, seed)
                    age[name], frames[name], rebased[name] = 0, [], []
                else:
                    pool.close_slot(slot_of.pop(name))
            ctrl = {}
            for name, slot in slot_of.items():
                x, mouse, btn, _ = ses[name]
                i = x.size(1) + age[name]
                ctrl[slot] = (mouse[:, i:i + 1], btn[:, i:i + 1])
            before = list(pool.rebases)
            out = pool.step(ctrl)
            assert sorted(out) == sorted(ctrl)
            for name, slot in slot_of.items():
                frames[name].append(out[slot])
                age[name] += 1
                if pool.rebases[slot] > before[slot]:
                    rebased[name].append(tick)
        state = pool.kv_cache.host_state()
        assert pool.kv_cache.device_state() == state
        bufs1 = bufs(pool)
    torch.cuda.synchronize()
    info = dict(slots=slots, rebased=rebased, state=state, pool=pool, bufs0=bufs0, bufs1=bufs1)
    return {n: torch.cat(f, 1) for n, f in frames.items()}, info


def _generator_matches_default(seed, shapes):
    """a fresh device generator seeded `seed` draws what the default generator draws after manual_seed(seed)"""
    torch.manual_seed(seed)
    a = [torch.randn(s, device="cuda", dtype=torch.bfloat16) for s in shapes]
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    b = [torch.randn(s, generator=g, device="cuda", dtype=torch.bfloat16) for s in shapes]
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _seed_default_like_session(seed, shapes):
    """the default generator in the state of a session's generator seeded `seed`"""
    if _generator_matches_default(seed, shapes):
        torch.manual_seed(seed)
    else:  # this torch build seeds the two differently: hand over the session generator's state itself
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        torch.cuda.set_rng_state(g.get_state())


@functools.lru_cache(maxsize=None)
def single_stream(name, frames, d_model, cfg_scale, max_cached_frames, n_frames=32):
    """the session alone on a B = 1 FrameStream (eager; its graph modes give the same bits,
    tests/test_stream_gpu.py, tests/test_frame_graph_gpu.py)"""
    from owl_wms.sampling.stream import FrameStream
    x, mouse, btn, seed = sessions()[name]
    init = x.size(1)
    _seed_default_like_session(seed, [tuple(x.shape), (1, 1, *x.shape[2:]), (1, 1, *x.shape[2:])])
    with FrameStream(_model(d_model, n_frames).core, cfg_scale=cfg_scale, max_cached_frames=max_cached_frames,
                     **KW) as s:
        s.start(x, mouse, btn)
        out = [s.step(mouse[:, init + i:init + i + 1], btn[:, init + i:init + i + 1]) for i in range(frames)]
    return torch.cat(out, 1)


def test_session_generator_reproduces_the_default_generator():
    """the premise of the FrameStream comparisons, on plain randn calls of the streams' shapes"""
    assert _generator_matches_default(321, [(1, 3, 32, 8, 8), (1, 1, 32, 8, 8), (1, 1, 32, 8, 8), (1, 1, 32, 8, 8)])


@pytest.mark.parametrize("graphed", MODES)
@pytest.mark.parametrize("cfg_scale", [1.3, 1.0])
@pytest.mark.parametrize("d_model", [128, 256])
def test_one_slot_is_frame_stream(d_model, cfg_scale, graphed):
    """n_slots 1, 3 context frames, max_cached_frames 6, 14 frames (the 7-frame ring wraps twice): the bits
    of a B = 1 FrameStream with the same seed."""
    ref = single_stream("A", 14, d_model, cfg_scale, 6)
    out, info = run_pool(_model(d_model, 32).core, 1, {0: [("open", "A")]}, 14, cfg_scale=cfg_scale,
                         max_cached_frames=6, graphed=graphed)
    assert out["A"].shape == ref.shape == (1, 14, 32, 8, 8) and torch.isfinite(ref.float()).all()
    assert torch.equal(out["A"], ref)
    pool = info["pool"]
    assert pool.frames_generated == [14] and pool.rebases == [0] and pool.ticks == 14
    assert info["state"] == [((11 * 64) % (7 * 64), 6 * 64, 17 * 64, 1)]  # 11 evictions on a 7-frame ring
    assert pool.graph_replays == {False: 0, True: 14 * 4 - 1, "frame": 13}[graphed]


ALONE = {0: [("open", "A")]}
JOINED = {0: [("open", "A")], 3: [("open", "B")], 6: [("open", "C")]}  # B after tick 2, C after tick 5
SECOND = {0: [("open", "X"), ("open", "A")], 5: [("close", "X")]}  # A in slot 1, slot 0 closed half-way


@functools.lru_cache(maxsize=None)
def three_slots(setting, d_model, graphed, max_cached_frames=6, n_frames=32, ticks=10):
    script = {"alone": ALONE, "joined": JOINED, "second": SECOND}[setting]
    return run_pool(_model(d_model, n_frames).core, 3, script, ticks, cfg_scale=1.3,
                    max_cached_frames=max_cached_frames, graphed=graphed)


@pytest.mark.parametrize("d_model", [128, 256])
def test_neighbours_and_slot_number_do_not_matter(d_model):
    """Session A alone in slot 0, in slot 0 with B and C joining later, and in slot 1 beside a session that
    leaves: its 10 frames bit for bit the same, in all three graph modes."""
    ref, _ = three_slots("alone", d_model, False)
    assert ref["A"].shape == (1, 10, 32, 8, 8)
    for setting in ("alone", "joined", "second"):
        for graphed in MODES:
            out, info = three_slots(setting, d_model, graphed)
            assert info["slots"]["A"] == (1 if setting == "second" else 0)
            assert torch.equal(out["A"], ref["A"]), (setting, graphed)
            for name, f in out.items():
                assert torch.isfinite(f.float()).all(), (setting, graphed, name)
    out, info = three_slots("joined", d_model, "frame")
    assert info["slots"] == {"A": 0, "B": 1, "C": 2}
    assert [out[n].shape[1] for n in "ABC"] == [10, 7, 4]
    a, b, c = info["state"]
    # A: 3 + 10 frames through a 7-frame ring; B: 2 + 7; C: 1 + 4, nothing evicted yet
    assert a == ((7 * 64) % (7 * 64), 6 * 64, 13 * 64, 1) and b == (3 * 64, 6 * 64, 9 * 64, 1)
    assert c == (0, 5 * 64, 5 * 64, 1)
    assert len({a[:3], b[:3], c[:3]}) == 3 and a[2] != b[2] != c[2]
    _, info = three_slots("second", d_model, "frame")
    assert info["state"][0] == (0, 0, 0, 0) and info["state"][1][3] == 1  # the closed slot is idle on both sides


@pytest.mark.parametrize("d_model", [128, 256])
def test_sessions_match_their_single_streams(d_model):
    """Each session of the joined pool against its own B = 1 FrameStream, same seed and controls: rel-L2 <=
    2e-2 (the GEMMs' split-K plan follows M, so no equality)."""
    out, _ = three_slots("joined", d_model, False)
    for name in "ABC":
        n = out[name].shape[1]
        ref = single_stream(name, n, d_model, 1.3, 6)
        r = rel(out[name], ref)
        print(f"pool session {name} vs its FrameStream, d_model {d_model}, {n} frames: rel-L2 {r:.3e}")
        assert r <= 2e-2, (name, r)


@pytest.mark.parametrize("d_model", [128, 256])
def test_slot_reuse_leaks_nothing(d_model):
    """A leaves after tick 6 and D takes its slot beside B: D's frames are those of D in a fresh pool in the
    same slot beside a live slot 1; buffers and state keep their addresses and sizes since construction."""
    core = _model(d_model, 32).core
    reuse = {0: [("open", "A"), ("open", "B")], 7: [("close", "A"), ("open", "D")]}
    fresh = {0: [("open", "D"), ("open", "B")]}
    for graphed in MODES:
        out, info = run_pool(core, 3, reuse, 12, cfg_scale=1.3, max_cached_frames=6, graphed=graphed)
        assert info["slots"] == {"A": 0, "B": 1, "D": 0} and out["D"].shape[1] == 5 and out["A"].shape[1] == 7
        want, winfo = run_pool(core, 3, fresh, 5, cfg_scale=1.3, max_cached_frames=6, graphed=graphed)
        assert winfo["slots"] == {"D": 0, "B": 1}
        assert torch.equal(out["D"], want["D"]), graphed
        assert info["bufs0"] == info["bufs1"] and len(info["bufs0"]) == 2 + 1
        assert all(b[2] == (6, 7 * 64, d_model) for b in info["bufs0"][:2]) and info["bufs0"][2][1] == (3, 4)
        assert info["pool"].frames_generated[0] == 5  # the slot's counter restarted with D


@pytest.mark.parametrize("d_model", [128, 256])
def test_slots_rebase_on_their_own(d_model):
    """8-frame table, max_cached_frames 4, A from tick 0 and X from tick 2 (3 and 4 context frames), 12 ticks:
    each slot rebases when ITS positions reach the table's end, at different ticks; the three modes agree bit
    for bit; each session within rel-L2 2e-2 of the same pool on a 32-frame table, which never rebases."""
    script = {0: [("open", "A")], 2: [("open", "X")]}
    runs = {g: run_pool(_model(d_model, 8).core, 3, script, 12, cfg_scale=1.3, max_cached_frames=4, graphed=g)
            for g in MODES}
    out, info = runs[False]
    # frames of offset before tick t: A 3 + t, X 4 + (t - 2); a slot rebases (to 4 cached frames) at offset 8
    assert info["rebased"] == {"A": [5, 9], "X": [6, 10]}
    assert info["pool"].rebases[:2] == [2, 2]
    for g in MODES[1:]:
        assert runs[g][1]["rebased"] == info["rebased"]
        for name in "AX":
            assert torch.equal(runs[g][0][name], out[name]), (g, name)
    ref, rinfo = run_pool(_model(d_model, 32).core, 3, script, 12, cfg_scale=1.3, max_cached_frames=4, graphed=False)
    assert rinfo["rebased"] == {"A": [], "X": []}
    for name in "AX":
        r = rel(out[name], ref[name])
        print(f"rebased pool session {name} vs a 32-frame table, d_model {d_model}: rel-L2 {r:.3e}")
        assert torch.isfinite(out[name].float()).all() and r <= 2e-2, (name, r)


def test_pool_errors():
    from owl_wms.sampling.stream_pool import StreamPool
    core = _model(128, 32).core
    ses = sessions()
    with StreamPool(core, 2, cfg_scale=1.3, max_cached_frames=3, **KW) as pool:
        assert pool.step({}) == {} and pool.live == []
        with pytest.raises(ValueError, match="context frames"):
            pool.open(*ses["X"])  # 4 context frames, max_cached_frames 3
        a = pool.open(*ses["A"])
        assert a == 0 and pool.live == [0]
        x, mouse, btn, _ = ses["A"]
        c = (mouse[:, 3:4], btn[:, 3:4])
        with pytest.raises(ValueError, match="live slots"):
            pool.step({})  # the live slot's controls are missing
        with pytest.raises(ValueError, match="live slots"):
            pool.step({0: c, 1: c})  # an idle slot's controls
        with pytest.raises(ValueError, match="not live"):
            pool.close_slot(1)
        with pytest.raises(RuntimeError, match="open"):
            pool.start(x, mouse, btn)
        b = pool.open(*ses["B"])
        assert b == 1
        with pytest.raises(RuntimeError, match="slots are live"):
            pool.open(*ses["C"])
        out = pool.step({0: c, 1: (ses["B"][1][:, 2:3], ses["B"][2][:, 2:3])})
        assert sorted(out) == [0, 1] and all(torch.isfinite(f.float()).all() for f in out.values())
        pool.close_slot(0)
        assert pool.open(*ses["C"]) == 0  # the lowest free slot again
