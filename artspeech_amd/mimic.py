"""Prosody transfer: warp a synthesis onto a recording and speak like it (include/artspeech_hip.h: as_dtw_f32, as_dtw_features_f32,
as_transfer_rows_f32; the rule: csrc/dtw_rule.h).

``dtw`` aligns a caller's dense cost, ``dtw_features`` two packed feature sets by device offsets, ``transfer_rows`` turns the warp's rows
into one prosody row per token (ArtSpeech's ``token_prosody``); ``Transfer`` names what is taken over.  The ``*_host`` twins run the same
rule on numpy arrays without a GPU.  Nothing here reads a device value back or synchronises.
"""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_T, MAX_C = _lib.AS_DTW_MAX_T, _lib.AS_DTW_MAX_C


class Transfer:
    """What pass B takes from the recording: each 0 (nothing) .. 1 (all of the measured difference); timing is on or off."""

    def __init__(self, timing=1, pitch=1, energy=1, ema=0):
        for name, v in (("timing", timing), ("pitch", pitch), ("energy", energy), ("ema", ema)):
            if not (float(v) >= 0.0) or float(v) == float("inf"):
                raise ValueError(f"Transfer: {name} must be a finite number >= 0")
        self.timing, self.pitch, self.energy, self.ema = float(timing), float(pitch), float(energy), float(ema)

    @classmethod
    def of_tracks(cls, names):
        """from a list of names among timing, pitch, energy, ema (the command line's --like-tracks)"""
        names = [n.strip() for n in names if n.strip()]
        bad = sorted(set(names) - {"timing", "pitch", "energy", "ema"})
        if bad:
            raise ValueError(f"Transfer: unknown track(s) {', '.join(bad)} (timing, pitch, energy, ema)")
        return cls(**{k: float(k in names) for k in ("timing", "pitch", "energy", "ema")})

    def strengths(self):
        """the 13 values of as_transfer_io.strength: timing, then F0, N, EMA0..9"""
        return [self.timing, self.pitch, self.energy] + [self.ema] * 10


def _strengths(transfer):
    """a Transfer, None (the default Transfer) or 13 numbers -> the C array of as_transfer_io.strength"""
    v = Transfer().strengths() if transfer is None else transfer.strengths() if isinstance(transfer, Transfer) else [float(x) for x in transfer]
    if len(v) != 13:
        raise ValueError("transfer: a Transfer or 13 strengths (timing, F0, N, EMA0..9)")
    return (ctypes.c_float * 13)(*v)


_WS = {}                            # (device index, B, Tx, Ty) -> workspace: the same one at every call, as a captured graph needs


def _workspace(dev, B, Tx, Ty):
    key = (dev.index, B, Tx, Ty)
    ws = _WS.get(key)
    if ws is None:
        n = _lib.lib().as_dtw_workspace_bytes(B, Tx, Ty)
        if n == 0:
            raise ValueError(f"dtw: B >= 1 and capacities in [1, {MAX_T}] (got B = {B}, Tx = {Tx}, Ty = {Ty})")
        ws = _WS[key] = torch.empty(n, dtype=torch.uint8, device=dev)
    return ws


def _need(t, dtype, what):
    if not torch.is_tensor(t) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {dtype} tensor on the GPU")
    return t


def _outputs(dev, B, Tx, Ty):
    return (torch.empty(B, Ty, dtype=torch.int32, device=dev), torch.empty(B, Tx, dtype=torch.int32, device=dev),
            torch.zeros(B, dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev))


def dtw(cost, t_x, t_y):
    """cost fp32 [B][Tx][Ty], t_x / t_y int32 [B], all on the device -> (rows int32 [B][Ty], cols int32 [B][Tx], total fp32 [B], steps
    int32 [B]); two launches on the current stream"""
    _need(cost, torch.float32, "dtw: cost")
    _need(t_x, torch.int32, "dtw: t_x")
    _need(t_y, torch.int32, "dtw: t_y")
    B, Tx, Ty = cost.shape
    dev = cost.device
    with torch.cuda.device(dev):
        rows, cols, total, steps = _outputs(dev, B, Tx, Ty)
        ws = _workspace(dev, B, Tx, Ty)
        _lib.check(_lib.lib().as_dtw_f32(_lib.ptr(cost), _lib.ptr(t_x), _lib.ptr(t_y), B, Tx, Ty, _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(total),
                                         _lib.ptr(steps), _lib.ptr(ws), ws.numel(), _lib.stream()), "as_dtw_f32")
    return rows, cols, total, steps


def dtw_features(a, a_off, b, b_off, Tx, Ty, a_mult=1, b_mult=1, center=True, cost_out=False):
    """a fp32 [C][lda] (the synthesis), b fp32 [C][ldb] (the recording), utterance u at the columns [mult off[u], mult off[u + 1]) of its
    side (off: device int32 [B + 1]); Tx, Ty: the frames there is room for per utterance -> (rows, cols, total, steps[, cost [B][Tx][Ty]]).
    Four launches; no host value is read."""
    _need(a, torch.float32, "dtw_features: a")
    _need(b, torch.float32, "dtw_features: b")
    _need(a_off, torch.int32, "dtw_features: a_off")
    _need(b_off, torch.int32, "dtw_features: b_off")
    if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[0] or a_off.numel() != b_off.numel():
        raise ValueError("dtw_features: a [C][lda] and b [C][ldb] with the same C, offsets of the same length")
    B, dev = a_off.numel() - 1, a.device
    with torch.cuda.device(dev):
        rows, cols, total, steps = _outputs(dev, B, Tx, Ty)
        cost = torch.zeros(B, Tx, Ty, dtype=torch.float32, device=dev) if cost_out else None
        ws = _workspace(dev, B, Tx, Ty)
        io = _lib.DtwIO(a=_lib.ptr(a), lda=a.shape[1], a_off=_lib.ptr(a_off), a_mult=int(a_mult), b=_lib.ptr(b), ldb=b.shape[1],
                        b_off=_lib.ptr(b_off), b_mult=int(b_mult), C=a.shape[0], B=B, Tx=int(Tx), Ty=int(Ty), center=int(bool(center)),
                        rows=_lib.ptr(rows), cols=_lib.ptr(cols), total=_lib.ptr(total), steps=_lib.ptr(steps), cost_out=_lib.ptr(cost))
        _lib.check(_lib.lib().as_dtw_features_f32(ctypes.byref(io), _lib.ptr(ws), ws.numel(), _lib.stream()), "as_dtw_features_f32")
    return (rows, cols, total, steps, cost) if cost_out else (rows, cols, total, steps)


def transfer_rows(rows, tok_off, dur_i, duration, F0, N, EMA, syn_off, feat12, rec_off, transfer=None, syn_mult=2, rec_mult=1, ld_out=25):
    """the warp's rows [B][Ty] + pass A's dur_i / duration [tokens], F0 / N [ld] and EMA [10][ld] (utterance u at syn_mult * syn_off[u]) + the
    recording's feat12 [12][ld_feat] (at rec_mult * rec_off[u]) -> (out_rows fp32 [tokens][ld_out] for token_prosody, target_dur int32
    [tokens], misses int32 [B]).  One launch."""
    for t, dt, what in ((rows, torch.int32, "rows"), (tok_off, torch.int32, "tok_off"), (dur_i, torch.int32, "dur_i"),
                        (duration, torch.float32, "duration"), (F0, torch.float32, "F0"), (N, torch.float32, "N"), (EMA, torch.float32, "EMA"),
                        (syn_off, torch.int32, "syn_off"), (feat12, torch.float32, "feat12"), (rec_off, torch.int32, "rec_off")):
        _need(t, dt, "transfer_rows: " + what)
    B, dev, n_tok = tok_off.numel() - 1, rows.device, dur_i.numel()
    ld_pred = F0.shape[-1]
    if N.shape[-1] != ld_pred or EMA.shape[-1] != ld_pred or EMA.numel() != 10 * ld_pred or feat12.shape[0] != 12:
        raise ValueError("transfer_rows: F0 [ld], N [ld], EMA [10][ld] with one ld; feat12 [12][ld_feat]")
    with torch.cuda.device(dev):
        out = torch.zeros(n_tok, ld_out, dtype=torch.float32, device=dev)
        target = torch.zeros(n_tok, dtype=torch.int32, device=dev)
        misses = torch.zeros(B, dtype=torch.int32, device=dev)
        io = _lib.TransferIO(B=B, rows=_lib.ptr(rows), ld_rows=rows.shape[-1], tok_off=_lib.ptr(tok_off), tok_cap=n_tok, dur_i=_lib.ptr(dur_i),
                             duration=_lib.ptr(duration), F0=_lib.ptr(F0), N=_lib.ptr(N), EMA=_lib.ptr(EMA), ld_pred=ld_pred,
                             syn_off=_lib.ptr(syn_off), syn_mult=int(syn_mult), feat12=_lib.ptr(feat12), ld_feat=feat12.shape[1],
                             rec_off=_lib.ptr(rec_off), rec_mult=int(rec_mult), strength=_strengths(transfer),
                             out_rows=_lib.ptr(out), ld_out=int(ld_out), target_dur=_lib.ptr(target), misses=_lib.ptr(misses))
        _lib.check(_lib.lib().as_transfer_rows_f32(ctypes.byref(io), _lib.stream()), "as_transfer_rows_f32")
    return out, target, misses


# ---- the same rule on host arrays (no GPU) ------------------------------------------------------------------------------------------
def _at(a):
    return None if a is None else a.ctypes.data


def dtw_host(cost, t_x, t_y):
    """as_dtw_host on numpy arrays -> (rows, cols, total, steps); total and steps of an empty utterance stay 0"""
    cost = np.ascontiguousarray(cost, np.float32)
    t_x, t_y = np.ascontiguousarray(t_x, np.int32), np.ascontiguousarray(t_y, np.int32)
    B, Tx, Ty = cost.shape
    rows, cols = np.empty((B, Ty), np.int32), np.empty((B, Tx), np.int32)
    total, steps = np.zeros(B, np.float32), np.zeros(B, np.int32)
    _lib.check(_lib.lib().as_dtw_host(_at(cost), _at(t_x), _at(t_y), B, Tx, Ty, _at(rows), _at(cols), _at(total), _at(steps)), "as_dtw_host")
    return rows, cols, total, steps


def dtw_features_host(a, a_off, b, b_off, Tx, Ty, a_mult=1, b_mult=1, center=True):
    """as_dtw_features_host on numpy arrays -> (rows, cols, total, steps, cost [B][Tx][Ty]; cells outside a lattice are 0)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    a_off, b_off = np.ascontiguousarray(a_off, np.int32), np.ascontiguousarray(b_off, np.int32)
    B = a_off.size - 1
    rows, cols = np.empty((B, Ty), np.int32), np.empty((B, Tx), np.int32)
    total, steps, cost = np.zeros(B, np.float32), np.zeros(B, np.int32), np.zeros((B, Tx, Ty), np.float32)
    io = _lib.DtwIO(a=_at(a), lda=a.shape[1], a_off=_at(a_off), a_mult=int(a_mult), b=_at(b), ldb=b.shape[1], b_off=_at(b_off),
                    b_mult=int(b_mult), C=a.shape[0], B=B, Tx=int(Tx), Ty=int(Ty), center=int(bool(center)), rows=_at(rows), cols=_at(cols),
                    total=_at(total), steps=_at(steps), cost_out=_at(cost))
    _lib.check(_lib.lib().as_dtw_features_host(ctypes.byref(io)), "as_dtw_features_host")
    return rows, cols, total, steps, cost


def transfer_rows_host(rows, tok_off, dur_i, duration, F0, N, EMA, syn_off, feat12, rec_off, transfer=None, syn_mult=2, rec_mult=1, ld_out=25):
    """as_transfer_rows_host on numpy arrays -> (out_rows, target_dur, misses)"""
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    f32 = lambda v: np.ascontiguousarray(v, np.float32)
    rows, tok_off, dur_i, syn_off, rec_off = i32(rows), i32(tok_off), i32(dur_i), i32(syn_off), i32(rec_off)
    duration, F0, N, EMA, feat12 = f32(duration), f32(F0), f32(N), f32(EMA), f32(feat12)
    B, n_tok, ld_pred = tok_off.size - 1, dur_i.size, F0.shape[-1]
    out = np.zeros((n_tok, ld_out), np.float32)
    target, misses = np.zeros(n_tok, np.int32), np.zeros(B, np.int32)
    io = _lib.TransferIO(B=B, rows=_at(rows), ld_rows=rows.shape[-1], tok_off=_at(tok_off), tok_cap=n_tok, dur_i=_at(dur_i), duration=_at(duration),
                         F0=_at(F0), N=_at(N), EMA=_at(EMA), ld_pred=ld_pred, syn_off=_at(syn_off), syn_mult=int(syn_mult), feat12=_at(feat12),
                         ld_feat=feat12.shape[1], rec_off=_at(rec_off), rec_mult=int(rec_mult),
                         strength=_strengths(transfer), out_rows=_at(out), ld_out=int(ld_out), target_dur=_at(target),
                         misses=_at(misses))
    _lib.check(_lib.lib().as_transfer_rows_host(ctypes.byref(io)), "as_transfer_rows_host")
    return out, target, misses
