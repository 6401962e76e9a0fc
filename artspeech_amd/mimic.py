"""Prosody transfer: warp a synthesis onto a recording and speak like it (include/artspeech_hip.h: as_dtw_f32, as_dtw_features_f32,
as_transfer_rows_f32; the rule: csrc/dtw_rule.h).

``dtw`` aligns a caller's dense cost, ``dtw_features`` two packed feature sets by device offsets, ``transfer_rows`` turns the warp's rows
into one prosody row per token (ArtSpeech's ``token_prosody``); ``Transfer`` names what is taken over.  The ``*_host`` twins run the same
rule on numpy arrays without a GPU.  Nothing here reads a device value back or synchronises.
"""
import ctypes

import torch

from . import _lib, stage

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


_WS = stage.Workspaces()            # keyed by (B, Tx, Ty)


def _workspace(dev, B, Tx, Ty):
    return _WS.get(dev, (B, Tx, Ty), lambda: _lib.lib().as_dtw_workspace_bytes(B, Tx, Ty),
                   f"dtw: B >= 1 and capacities in [1, {MAX_T}] (got B = {B}, Tx = {Tx}, Ty = {Ty})")


class _Device(stage.Device):
    __slots__ = ()
    names = {d: str(d) for d in stage.Device.names}         # (these messages have always named a dtype as torch prints it)


def _on(t):
    """the device rule where t lives (the fillers refuse what is no tensor on a GPU)"""
    return _Device(t.device if torch.is_tensor(t) else None)


def _outputs(r, B, Tx, Ty):
    """rows, cols, total, steps: total and steps of an empty utterance stay 0"""
    return r.empty((B, Ty), stage.I32), r.empty((B, Tx), stage.I32), r.zeros(B, stage.F32), r.zeros(B, stage.I32)


# ---- one filler per call, under the array rule r (_Device / stage.Host) ---------------------------------------------------------------
def _dtw_args(r, cost, t_x, t_y):
    """-> (what as_dtw_f32 and as_dtw_host take in front of a workspace, (B, Tx, Ty), the outputs)"""
    cost, t_x, t_y = r.need(cost, stage.F32, "dtw", "cost"), r.need(t_x, stage.I32, "dtw", "t_x"), r.need(t_y, stage.I32, "dtw", "t_y")
    B, Tx, Ty = cost.shape
    out = _outputs(r, B, Tx, Ty)
    return (r.at(cost), r.at(t_x), r.at(t_y), B, Tx, Ty) + tuple(r.at(o) for o in out), (B, Tx, Ty), out


def _dtw_io(r, a, a_off, b, b_off, Tx, Ty, a_mult, b_mult, center, cost_out):
    """-> (as_dtw_io, B, the outputs rows, cols, total, steps, cost or None)"""
    a, b = r.need(a, stage.F32, "dtw_features", "a"), r.need(b, stage.F32, "dtw_features", "b")
    a_off, b_off = r.need(a_off, stage.I32, "dtw_features", "a_off"), r.need(b_off, stage.I32, "dtw_features", "b_off")
    if a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0] or r.count(a_off) != r.count(b_off):
        raise ValueError("dtw_features: a [C][lda] and b [C][ldb] with the same C, offsets of the same length")
    B = r.count(a_off) - 1
    out = _outputs(r, B, Tx, Ty) + (r.zeros((B, Tx, Ty), stage.F32) if cost_out else None,)
    rows, cols, total, steps, cost = out
    io = _lib.DtwIO(a=r.at(a), lda=a.shape[1], a_off=r.at(a_off), a_mult=int(a_mult), b=r.at(b), ldb=b.shape[1], b_off=r.at(b_off),
                    b_mult=int(b_mult), C=a.shape[0], B=B, Tx=int(Tx), Ty=int(Ty), center=int(bool(center)), rows=r.at(rows), cols=r.at(cols),
                    total=r.at(total), steps=r.at(steps), cost_out=r.at(cost))
    return io, B, out


def _transfer_io(r, rows, tok_off, dur_i, duration, F0, N, EMA, syn_off, feat12, rec_off, transfer, syn_mult, rec_mult, ld_out):
    """-> (as_transfer_io, the outputs out_rows, target_dur, misses)"""
    rows, tok_off, dur_i, syn_off, rec_off = (r.need(t, stage.I32, "transfer_rows", name) for t, name in (
        (rows, "rows"), (tok_off, "tok_off"), (dur_i, "dur_i"), (syn_off, "syn_off"), (rec_off, "rec_off")))
    duration, F0, N, EMA, feat12 = (r.need(t, stage.F32, "transfer_rows", name) for t, name in (
        (duration, "duration"), (F0, "F0"), (N, "N"), (EMA, "EMA"), (feat12, "feat12")))
    B, n_tok, ld_pred = r.count(tok_off) - 1, r.count(dur_i), F0.shape[-1]
    if N.shape[-1] != ld_pred or EMA.shape[-1] != ld_pred or r.count(EMA) != 10 * ld_pred or feat12.shape[0] != 12:
        raise ValueError("transfer_rows: F0 [ld], N [ld], EMA [10][ld] with one ld; feat12 [12][ld_feat]")
    out = r.zeros((n_tok, ld_out), stage.F32), r.zeros(n_tok, stage.I32), r.zeros(B, stage.I32)
    io = _lib.TransferIO(B=B, rows=r.at(rows), ld_rows=rows.shape[-1], tok_off=r.at(tok_off), tok_cap=n_tok, dur_i=r.at(dur_i),
                         duration=r.at(duration), F0=r.at(F0), N=r.at(N), EMA=r.at(EMA), ld_pred=ld_pred, syn_off=r.at(syn_off),
                         syn_mult=int(syn_mult), feat12=r.at(feat12), ld_feat=feat12.shape[1], rec_off=r.at(rec_off), rec_mult=int(rec_mult),
                         strength=_strengths(transfer), out_rows=r.at(out[0]), ld_out=int(ld_out), target_dur=r.at(out[1]), misses=r.at(out[2]))
    return io, out


# ---- on the device ------------------------------------------------------------------------------------------------------------------
def dtw(cost, t_x, t_y):
    """cost fp32 [B][Tx][Ty], t_x / t_y int32 [B], all on the device -> (rows int32 [B][Ty], cols int32 [B][Tx], total fp32 [B], steps
    int32 [B]); two launches on the current stream"""
    r = _on(cost)
    args, shape, out = _dtw_args(r, cost, t_x, t_y)
    with torch.cuda.device(r.dev):
        ws = _workspace(r.dev, *shape)
        _lib.check(_lib.lib().as_dtw_f32(*args, _lib.ptr(ws), ws.numel(), _lib.stream()), "as_dtw_f32")
    return out


def dtw_features(a, a_off, b, b_off, Tx, Ty, a_mult=1, b_mult=1, center=True, cost_out=False):
    """a fp32 [C][lda] (the synthesis), b fp32 [C][ldb] (the recording), utterance u at the columns [mult off[u], mult off[u + 1]) of its
    side (off: device int32 [B + 1]); Tx, Ty: the frames there is room for per utterance -> (rows, cols, total, steps[, cost [B][Tx][Ty]]).
    Four launches; no host value is read."""
    r = _on(a)
    io, B, out = _dtw_io(r, a, a_off, b, b_off, Tx, Ty, a_mult, b_mult, center, cost_out)
    with torch.cuda.device(r.dev):
        ws = _workspace(r.dev, B, Tx, Ty)
        _lib.check(_lib.lib().as_dtw_features_f32(ctypes.byref(io), _lib.ptr(ws), ws.numel(), _lib.stream()), "as_dtw_features_f32")
    return out if cost_out else out[:4]


def transfer_rows(rows, tok_off, dur_i, duration, F0, N, EMA, syn_off, feat12, rec_off, transfer=None, syn_mult=2, rec_mult=1, ld_out=25):
    """the warp's rows [B][Ty] + pass A's dur_i / duration [tokens], F0 / N [ld] and EMA [10][ld] (utterance u at syn_mult * syn_off[u]) + the
    recording's feat12 [12][ld_feat] (at rec_mult * rec_off[u]) -> (out_rows fp32 [tokens][ld_out] for token_prosody, target_dur int32
    [tokens], misses int32 [B]).  One launch."""
    r = _on(rows)
    io, out = _transfer_io(r, rows, tok_off, dur_i, duration, F0, N, EMA, syn_off, feat12, rec_off, transfer, syn_mult, rec_mult, ld_out)
    with torch.cuda.device(r.dev):
        _lib.check(_lib.lib().as_transfer_rows_f32(ctypes.byref(io), _lib.stream()), "as_transfer_rows_f32")
    return out


# ---- the same rule on host arrays (no GPU) ------------------------------------------------------------------------------------------
def dtw_host(cost, t_x, t_y):
    """as_dtw_host on numpy arrays -> (rows, cols, total, steps); total and steps of an empty utterance stay 0"""
    args, _, out = _dtw_args(stage.Host(), cost, t_x, t_y)
    _lib.check(_lib.lib().as_dtw_host(*args), "as_dtw_host")
    return out


def dtw_features_host(a, a_off, b, b_off, Tx, Ty, a_mult=1, b_mult=1, center=True):
    """as_dtw_features_host on numpy arrays -> (rows, cols, total, steps, cost [B][Tx][Ty]; cells outside a lattice are 0)"""
    io, _, out = _dtw_io(stage.Host(), a, a_off, b, b_off, Tx, Ty, a_mult, b_mult, center, True)
    _lib.check(_lib.lib().as_dtw_features_host(ctypes.byref(io)), "as_dtw_features_host")
    return out


def transfer_rows_host(rows, tok_off, dur_i, duration, F0, N, EMA, syn_off, feat12, rec_off, transfer=None, syn_mult=2, rec_mult=1, ld_out=25):
    """as_transfer_rows_host on numpy arrays -> (out_rows, target_dur, misses)"""
    io, out = _transfer_io(stage.Host(), rows, tok_off, dur_i, duration, F0, N, EMA, syn_off, feat12, rec_off, transfer, syn_mult, rec_mult, ld_out)
    _lib.check(_lib.lib().as_transfer_rows_host(ctypes.byref(io)), "as_transfer_rows_host")
    return out
