"""The gradient guard's host side, no GPU: the config keys, the C entry's refusals (made before any HIP
call) and its workspace arithmetic, and the reducer's cross-rank finite flag on gloo."""
import ctypes
import glob
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import yaml

from conftest import REPO

CHUNK = 1 << 16  # elements per workgroup (include/owlk.h, owlk_grad_guard)


def test_training_config_defaults():
    from owl_wms.configs import TrainingConfig, make_section
    c = make_section(TrainingConfig, {})
    assert c.grad_guard is False and c.grad_clip_norm == 10.0 and c.max_consecutive_skips is None


def test_no_shipped_config_turns_the_guard_on():
    from owl_wms.configs import Config
    files = sorted(glob.glob(os.path.join(REPO, "configs", "*.yml")))
    assert files
    for f in files:
        assert "grad_guard" not in (yaml.safe_load(open(f)).get("train") or {}), f
        c = Config.from_yaml(f).train
        assert c.grad_guard is False and c.grad_clip_norm == 10.0, f


def _lib():
    from owl_wms import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libowlk.so not built (run __graft_entry__.build())")
    return _lib


def _longs(ns):
    return (ctypes.c_long * len(ns))(*ns)


def _ptrs(ps):
    return (ctypes.c_void_p * len(ps))(*ps)


def test_workspace_query_is_a_function_of_the_lengths():
    """one fp32 partial per 65536-element chunk of each buffer, whatever the machine"""
    q = _lib().lib().owlk_grad_guard_ws_bytes
    assert q(0, None) == 0
    assert q(3, _longs([0, 0, 0])) == 0
    assert q(1, _longs([1])) == 4
    assert q(4, _longs([CHUNK, CHUNK + 1, 0, 5])) == 4 * (1 + 2 + 0 + 1)
    assert q(1, _longs([705_000_000])) == 4 * ((705_000_000 + CHUNK - 1) // CHUNK)
    assert q(2, _longs([8, -1])) == 0  # a bad length: nothing to allocate, the entry itself refuses


# stand-in addresses: nothing is dereferenced, every check fails first
@pytest.mark.parametrize("args,msg", [
    ((1, None, _longs([8]), 0.0, 4096, 8192, 4, None), "g, n and state are required"),
    ((1, _ptrs([4096]), _longs([8]), 0.0, None, 8192, 4, None), "g, n and state are required"),
    ((1, _ptrs([4096]), _longs([8]), 0.0, 4100, 8192, 4, None), "state must be 16-byte aligned"),
    ((2, _ptrs([4096, 8192]), _longs([8, -3]), 0.0, 4096, 8192, 8, None), "buffer 1 has negative length -3"),
    ((2, _ptrs([4096, None]), _longs([8, 8]), 0.0, 4096, 8192, 8, None), "buffer 1 is a null pointer"),
    ((2, _ptrs([4096, 8200]), _longs([8, 8]), 1.0, 4096, 8192, 8, None), "buffer 1 must be 16-byte aligned"),
    ((2, _ptrs([4096, 8192]), _longs([8, 8]), 1.0, 4096, 8192, 4, None), "asks for 8"),
    ((2, _ptrs([4096, 8192]), _longs([8, 8]), 1.0, 4096, 8194, 8, None), "4-byte aligned"),
    ((2, _ptrs([4096, 8192]), _longs([8, 8]), 1.0, 4096, None, 8, None), "workspace of 8 bytes"),
])
def test_c_entry_refuses_before_any_hip_call(args, msg):
    L = _lib()
    assert L.lib().owlk_grad_guard(*args) != 0
    assert msg in L.lib().owlk_last_error().decode()
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        L.call("owlk_grad_guard", *args)


def test_binding_refuses_host_tensors():
    from owl_wms import kernels as K
    with pytest.raises(RuntimeError, match="buffer 0 must be a device tensor"):
        K.grad_guard([torch.zeros(8)])


# ------------------------------------------------------------------ world_size 2 on gloo
def _torch_guard(bufs, max_norm=None):
    """kernels.grad_guard restated in torch for host tensors: [norm, clip_coef, finite, 0]"""
    s = sum(b.double().pow(2).sum() for b in bufs)
    finite = bool(torch.isfinite(s))
    norm = s.sqrt().float()
    coef = torch.ones(())
    if finite and max_norm:
        coef = (max_norm / (norm + 1e-6)).clamp(max=1.0)
        for b in bufs:
            b.mul_(coef)
    return torch.stack([norm, coef, torch.tensor(float(finite)), torch.zeros(())]).float()


def _worker(rank, ws, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        import owl_wms.kernels as K
        from owl_wms.utils.grad_reducer import GradReducer
        K.grad_guard = _torch_guard
        torch.manual_seed(0)
        model = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.SiLU(), torch.nn.Linear(32, 8))
        red = GradReducer(model.parameters(), bucket_mb=0.001, world_size=ws)
        for poison in (False, True):
            red.zero_grad()
            red.begin(sync=True)
            model(torch.randn(4, 16)).pow(2).mean().backward()
            red.finish()
            if poison and rank == 1:  # after the all-reduce: this rank's bucket alone is bad
                red.flat[0][0] = float("nan")
            res = red.grad_guard(max_norm=10.0)
            q.put((rank, poison, res.finite, res.norm, len(red.flat)))
    finally:
        dist.destroy_process_group()


def test_finite_flag_is_shared_by_the_ranks():
    ws = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [ctx.Process(target=_worker, args=(r, ws, port, q)) for r in range(ws)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2 * ws)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert all(r[4] > 1 for r in res)  # several buckets
    clean = {r[0]: r for r in res if not r[1]}
    bad = {r[0]: r for r in res if r[1]}
    assert clean[0][2] is True and clean[1][2] is True
    assert clean[0][3] == clean[1][3] and clean[0][3] > 0
    assert bad[0][2] is False and bad[1][2] is False  # rank 0's own buckets are finite
    assert bad[0][3] == bad[0][3] and bad[1][3] != bad[1][3]  # the norm is each rank's own: NaN on rank 1 only
