"""GPU: the job search of packed streams (artspeech_amd/csrc/packed_streams.h: find_job) with MORE STREAMS THAN SEARCHING THREADS, so that
a thread owns a run of two or more streams and the last threads' runs are empty: mastering at G = 65 and 300 (64 threads search in the
filter launches, 256 in the limiter), the joiner and the resampler at B = 257 and 600 (256 threads).  Every result is compared bit for bit
with the library's own host evaluation of the rule (as_master_host, as_join_host, resample_rule.h through the probe of
test_resample_cpu.py); offsets beyond the capacity raise AS_STATUS_CAPACITY, leave the guard bands intact and the next call clean."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, master, resample

import master_ref
from test_join_cpu import cfg_of as join_cfg_of, joiner_of
from test_master_cpu import cfg_of as master_cfg_of, pcm_rule
from test_master_gpu import device as master_device
from test_resample_cpu import ROOT, run_probe

pytestmark = pytest.mark.gpu
STATUS_CAPACITY = 1 << 5
GUARD = 64
bits = lambda a: np.ascontiguousarray(a).view(np.int32)


def lengths(count, special, seed):
    """`count` stream lengths from a fixed seed: 0 at the first, the last and two inner places, every length of `special` at a place of
    its own, the rest between 1 and 700"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 701, count)
    inner = rng.permutation(np.arange(1, count - 1))[: 2 + len(special)]
    lens[[0, count - 1, inner[0], inner[1]]] = 0
    lens[inner[2:]] = special
    return lens.astype(np.int64)


def samples(lens, seed, scale):
    """noise under a slow envelope, packed; off int32"""
    rng = np.random.default_rng(seed)
    n = int(lens.sum())
    env = np.repeat(rng.uniform(0.05, 1.0, n // 200 + 1), 200)[:n]
    return (scale * env * rng.standard_normal(n)).astype(np.float32), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


# ---- mastering: one tile and one tile + 1 of the limiter, 64 and 65 chunks of the filter (one workgroup full, and one chunk in the next)
MASTER_SPECIAL = [2048, 2049, 64 * 512, 64 * 512 + 1]
MASTER_CFG = dict(target_power=master.power_of_lufs(-20.0), max_gain=8.0, ceiling=0.5, lookahead=48)


@functools.lru_cache(maxsize=None)
def master_case(G):
    lens = lengths(G, MASTER_SPECIAL, 100 + G)
    assert sorted(lens[lens > 700].tolist()) == MASTER_SPECIAL and (lens[[0, -1]] == 0).all() and (lens == 0).sum() == 4
    return samples(lens, 200 + G, 0.3)


@pytest.mark.parametrize("G", [65, 300])
def test_master_with_more_streams_than_searching_threads(cuda, G):
    """loudness and limiter on, fp32 + PCM + report, 100 samples of filler: the bits of as_master_host"""
    x, off = master_case(G)
    x = np.concatenate([x, np.zeros(100, np.float32)])
    cfg = master_cfg_of(master_ref.GPU_RATE, **MASTER_CFG)
    rc, y, p, rep, status = master_device(cuda, cfg, x, off)
    assert rc == 0 and status == 0
    hy, hp, hrep = master.Master.from_cfg(cfg).host(x, off, pcm=True)
    assert np.array_equal(bits(rep), bits(hrep.raw))
    assert np.array_equal(bits(y), bits(hy)) and np.array_equal(p, hp) and np.array_equal(p, pcm_rule(y))
    assert not y[off[-1]:].any() and not p[off[-1]:].any()
    assert np.abs(y).max() <= 0.5 * (1 + 2.0 ** -14) and (rep[:, 3] < 1).any() and len({float(v) for v in rep[:, 1]}) > 10


@pytest.mark.parametrize("G", [65, 300])
def test_master_offsets_beyond_the_capacity(cuda, G):
    """in_off[G] > in_cap: AS_STATUS_CAPACITY, the guard bands intact (asserted inside master_device), the next call clean"""
    x, off = master_case(G)
    cfg = master_cfg_of(master_ref.GPU_RATE, **MASTER_CFG)
    assert _lib.lib().as_device_status(0) == 0
    rc, y, p, rep, status = master_device(cuda, cfg, x[: len(x) - 1000], off, in_cap=len(x) - 1000)
    assert rc == 0 and status == STATUS_CAPACITY
    rc, y, p, rep, status = master_device(cuda, cfg, x, off)
    hy, hp, hrep = master.Master.from_cfg(cfg).host(x, off, pcm=True)
    assert rc == 0 and status == 0 and np.array_equal(bits(y), bits(hy)) and np.array_equal(bits(rep), bits(hrep.raw))


# ---- the joiner: tiles of 2048 outputs; five streams, the first one empty.  The level is OFF (target_rms = 0, every gain exactly 1, so
# the comparison of `gain` exercises nothing here): with target_rms = 0.2 the device's gain differs from as_join_host's by 1 or 2 ulp in a
# few utterances (B = 257: utterances 254 and 255), because join_rule::root is __fsqrt_rn on the device, which is not correctly rounded on
# gfx950 (a bare v_sqrt_f32).  What is under test here is the search, not the level.
JOIN_CFG = dict(frame=64, trim_ratio=float(np.float32(1e-3)), keep=32, fade=40, gap=100, lead=7, tail=11, target_rms=0.0, peak_ceiling=0.9, max_gain=10.0)


@functools.lru_cache(maxsize=None)
def join_case(B):
    # (keep + frame more than a tile: the kept ranges straddle the tile of 2048 as well)
    lens = lengths(B, [2048, 2049, 2048 + 96, 4096 + 1], 300 + B)
    x, off = samples(lens, 400 + B, 0.2)
    groups = [0, 0, B // 5, B // 2, B - 3, B]
    gaps = np.random.default_rng(500 + B).integers(-20, 300, B).astype(np.int32)
    j = joiner_of(JOIN_CFG)
    need = j.out_cap(x.size, B, G=5, gap=300)
    return x, off, groups, gaps, need, j.host(x, off, need, groups, gaps, pcm=True)


def join_device(cuda, x, off, groups, gaps, in_cap, out_cap):
    """as_join_f32 on outputs with NaN / sentinel guard bands on both sides -> (rc, y, pcm, out_off, piece, gain, status bits)"""
    L, c = _lib.lib(), join_cfg_of(JOIN_CFG)
    B = len(off) - 1
    with torch.cuda.device(cuda):
        dx = torch.from_numpy(x).to(cuda)
        doff, dgrp, dgap = (torch.tensor(np.asarray(v), dtype=torch.int32, device=cuda) for v in (off, groups, gaps))
        yb = torch.full((out_cap + 2 * GUARD,), float("nan"), device=cuda)
        pb = torch.full((out_cap + 2 * GUARD,), -21846, dtype=torch.int16, device=cuda)
        ob = torch.full((6 + 2 * GUARD,), -5, dtype=torch.int32, device=cuda)
        piece = torch.full((B + 2, 4), -5, dtype=torch.int32, device=cuda)
        gain = torch.full((B + 2,), 12345.0, device=cuda)
        ws = torch.empty(L.as_join_workspace_bytes(B, in_cap, ctypes.byref(c)), dtype=torch.uint8, device=cuda)
        io = _lib.JoinIO(in_off=doff.data_ptr(), in_cap=in_cap, x=dx.data_ptr(), G=5, group_off=dgrp.data_ptr(), gap=dgap.data_ptr(), out_cap=out_cap,
                         y=yb.data_ptr() + 4 * GUARD, pcm=pb.data_ptr() + 2 * GUARD, out_off=ob.data_ptr() + 4 * GUARD, piece=piece.data_ptr() + 16,
                         gain=gain.data_ptr() + 4)
        rc = L.as_join_f32(ctypes.byref(c), B, ctypes.byref(io), ws.data_ptr(), ws.numel(), _lib.stream())
        torch.cuda.synchronize()
        status = L.as_device_status(1)
        y, p, o, pc, g = (t.cpu().numpy() for t in (yb, pb, ob, piece, gain))
    assert np.isnan(y[:GUARD]).all() and np.isnan(y[GUARD + out_cap:]).all() and (p[:GUARD] == -21846).all() and (p[GUARD + out_cap:] == -21846).all()
    assert (o[:GUARD] == -5).all() and (o[GUARD + 6:] == -5).all() and (pc[[0, -1]] == -5).all() and (g[[0, -1]] == 12345.0).all()
    return rc, y[GUARD: GUARD + out_cap], p[GUARD: GUARD + out_cap], o[GUARD: GUARD + 6], pc[1: B + 1], g[1: B + 1], status


@pytest.mark.parametrize("B", [257, 600])
def test_join_with_more_utterances_than_searching_threads(cuda, B):
    """out_off, piece, samples and PCM: the bits of as_join_host; the status words are clear.  `gain` is compared too but NOT exercised:
    the level is off (JOIN_CFG above says why), every gain is 1"""
    x, off, groups, gaps, need, (hy, hp, ho, hpiece, hg) = join_case(B)
    rc, y, p, o, piece, gain, status = join_device(cuda, x, off, groups, gaps, x.size, need)
    assert rc == 0 and status == 0
    assert np.array_equal(o, ho) and o[1] == JOIN_CFG["lead"] + JOIN_CFG["tail"] and np.array_equal(piece, hpiece) and np.array_equal(bits(gain), bits(hg))
    assert np.array_equal(bits(y), bits(hy)) and np.array_equal(p, hp)
    assert (piece[:, 1] > piece[:, 0]).sum() > B // 2 and not y[o[-1]:].any()


@pytest.mark.parametrize("B", [257, 600])
def test_join_offsets_beyond_the_capacity(cuda, B):
    x, off, groups, gaps, need, (hy, hp, ho, hpiece, hg) = join_case(B)
    assert _lib.lib().as_device_status(0) == 0
    rc, *_, status = join_device(cuda, x[: x.size - 1000], off, groups, gaps, x.size - 1000, need)
    assert rc == 0 and status == STATUS_CAPACITY
    rc, y, p, o, piece, gain, status = join_device(cuda, x, off, groups, gaps, x.size, need)
    assert rc == 0 and status == 0 and np.array_equal(bits(y), bits(hy)) and np.array_equal(piece, hpiece)


# ---- the resampler: a handle's tile is 512, 1024 or 2048 outputs.  An output count of exactly a tile does not exist at every ratio, so
# for each of the three the mix holds the longest input that still fits the tile and the next one, which needs a second tile.
PAIRS = [(24000, 16000), (24000, 44100)]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("packed") / "resample_probe"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "artspeech_amd", "csrc"), os.path.join(ROOT, "tests", "resample_probe.cpp"),
                           "-o", str(exe)])
    return exe


_RESAMPLE = {}


def resample_case(probe, tmp_path, pair, B):
    if (pair, B) not in _RESAMPLE:
        L, M, H, taps = resample.design(pair[0], pair[1], taps=True)
        special = [n for T in (512, 1024, 2048) for n in (T * M // L, T * M // L + 1)]
        assert all(-(-(T * M // L) * L // M) <= T < -(-(T * M // L + 1) * L // M) for T in (512, 1024, 2048))
        x, off = samples(lengths(B, special, 600 + B), 700 + B, 0.3)
        y, out_off = run_probe(probe, tmp_path, pair, off, taps, x)
        _RESAMPLE[(pair, B)] = (x, off, y.copy(), out_off.copy())
    return _RESAMPLE[(pair, B)]


def resample_device(cuda, pair, x, off, in_cap, out_cap):
    """as_resample_f32 on outputs with guard bands on both sides -> (rc, y, pcm, out_off, status bits)"""
    L = _lib.lib()
    B = len(off) - 1
    with torch.cuda.device(cuda):
        h = resample._handle(cuda, *pair)
        dx, doff = torch.from_numpy(x).to(cuda), torch.from_numpy(off).to(cuda)
        yb = torch.full((out_cap + 2 * GUARD,), float("nan"), device=cuda)
        pb = torch.full((out_cap + 2 * GUARD,), -21846, dtype=torch.int16, device=cuda)
        ob = torch.full((B + 1 + 2 * GUARD,), -5, dtype=torch.int32, device=cuda)
        rc = L.as_resample_f32(h, B, doff.data_ptr(), in_cap, dx.data_ptr(), out_cap, yb.data_ptr() + 4 * GUARD, pb.data_ptr() + 2 * GUARD,
                               ob.data_ptr() + 4 * GUARD, _lib.stream())
        torch.cuda.synchronize()
        status = L.as_device_status(1)
        y, p, o = yb.cpu().numpy(), pb.cpu().numpy(), ob.cpu().numpy()
    assert np.isnan(y[:GUARD]).all() and np.isnan(y[GUARD + out_cap:]).all() and (p[:GUARD] == -21846).all() and (p[GUARD + out_cap:] == -21846).all()
    assert (o[:GUARD] == -5).all() and (o[GUARD + B + 1:] == -5).all()
    return rc, y[GUARD: GUARD + out_cap], p[GUARD: GUARD + out_cap], o[GUARD: GUARD + B + 1], status


@pytest.mark.parametrize("B", [257, 600])
@pytest.mark.parametrize("pair", PAIRS, ids=["24000-16000", "24000-44100"])
def test_resample_with_more_utterances_than_searching_threads(cuda, probe, tmp_path, pair, B):
    """out_off, samples and PCM: the bits of resample_rule.h evaluated on the host; 300 samples of filler; the status words are clear"""
    x, off, hy, ho = resample_case(probe, tmp_path, pair, B)
    need = int(ho[-1])
    rc, y, p, o, status = resample_device(cuda, pair, x, off, x.size, need + 300)
    assert rc == 0 and status == 0
    assert np.array_equal(o, ho) and np.array_equal(bits(y[:need]), bits(hy)) and np.array_equal(p, pcm_rule(y))
    assert not y[need:].any() and np.abs(y).max() > 0.1


@pytest.mark.parametrize("B", [257, 600])
def test_resample_offsets_beyond_the_capacity(cuda, probe, tmp_path, B):
    pair = PAIRS[1]
    x, off, hy, ho = resample_case(probe, tmp_path, pair, B)
    need = int(ho[-1])
    assert _lib.lib().as_device_status(0) == 0
    rc, *_, status = resample_device(cuda, pair, x[: x.size - 1000], off, x.size - 1000, need)
    assert rc == 0 and status == STATUS_CAPACITY
    rc, y, p, o, status = resample_device(cuda, pair, x, off, x.size, need)
    assert rc == 0 and status == 0 and np.array_equal(o, ho) and np.array_equal(bits(y), bits(hy))
