"""Fit to time (as_plan_set_fit, as_fit_durations_f32, as_fit_host) restated in Python integers, from the rule's text and not from
artspeech_amd/csrc/duration_fit.h: the durations every token gets, which spans are void, the stretch of a span -- and, as a second and
independent statement of the pinned tokens, the iterative procedure "pin every free token whose share is below one frame, share the rest
again, repeat".  Also the seeded cases the CPU and the GPU tests share."""
import functools
from fractions import Fraction

import numpy as np

D_MAX, MAX_COUNT, MAX_SPANS = 16384, 4096, 4096


def finite(v):
    """the durations kernel's test (csrc/elementwise.hip): |v| <= 3e38 in fp32"""
    v = np.float32(v)
    return bool(np.isfinite(v)) and abs(float(v)) <= float(np.float32(3.0e38))


def plain(v):
    """clamp(rint(v), 1, 16384), ties to even; a non-finite v gives 1"""
    if not finite(v):
        return 1
    return min(max(round(Fraction(float(np.float32(v)))), 1), D_MAX)


def weight(v):
    """llrint(min(max(v, 2^-8), 16384) * 65536), a non-finite v counting as 1"""
    x = Fraction(float(np.float32(v))) if finite(v) else Fraction(1)
    x = min(max(x, Fraction(1, 256)), Fraction(D_MAX))
    return round(x * 65536)


def pinned_iterative(u, Tp):
    """how many of the free weights u end at one frame when Tp frames are shared: pin, share again, repeat"""
    pinned = set()
    while True:
        active = [i for i in range(len(u)) if i not in pinned]
        R, Ua = Tp - len(pinned), sum(u[i] for i in active)
        new = [i for i in active if u[i] * R < Ua]
        if not new:
            return len(pinned)
        pinned.update(new)


def fit_span(v, lock, T):
    """one span's tokens -> (durations or None if void, detail)"""
    r = [plain(x) for x in v]
    free = [j for j in range(len(v)) if not lock[j]]
    Tp = T - sum(r[j] for j in range(len(v)) if lock[j])
    n = len(free)
    detail = dict(free=free, Tp=Tp, n=n, valid=False, scale=0)
    if n == 0:
        detail["valid"] = Tp == 0
        return (r if Tp == 0 else None), detail
    if Tp < n:
        return None, detail
    u = {j: weight(v[j]) for j in free}
    order = sorted(free, key=lambda j: (u[j], j))
    U = sum(u.values())
    P, k = 0, None
    for a, j in enumerate(order):
        if u[j] * (Tp - a) >= U - P:
            k = a
            break
        P += u[j]
    assert k is not None
    R, Us = Tp - k, U - P
    d = list(r)
    for j in order[:k]:
        d[j] = 1
    act = order[k:]
    q = {j: u[j] * R // Us for j in act}
    rem = {j: u[j] * R % Us for j in act}
    m = R - sum(q.values())
    assert m == 0 or 0 < m < len(act)
    for j in sorted(act, key=lambda j: (-rem[j], j))[:m]:
        q[j] += 1
    for j in act:
        d[j] = q[j]
    detail.update(u=u, k=k, R=R, Us=Us, active=act, order=order)
    if any(x > D_MAX for x in d):
        return None, detail
    detail.update(valid=True, scale=R * 65536 // Us)
    return d, detail


def fit(v, tok_off, span_tok, span_frames, lock, max_count):
    """-> dict(dur [n_tokens], scale [n_spans], ok: no span void, range_ok: every v finite, details: per span or None)"""
    v = np.asarray(v, np.float32)
    n_tokens, B = len(v), len(tok_off) - 1
    dur = [plain(x) for x in v]
    lock = [0] * n_tokens if lock is None else [int(x) for x in lock]
    res = dict(dur=dur, scale=[0] * len(span_tok), ok=True, range_ok=all(finite(x) for x in v), details=[None] * len(span_tok))
    end = 0
    for first, count in span_tok:
        if first < 0 or count < 1 or first + count > min(n_tokens, tok_off[B]) or first < end:
            res["ok"] = False
            return res
        end = first + count
    for s, (first, count) in enumerate(span_tok):
        b = max(x for x in range(B) if tok_off[x] <= first)
        good = count <= max_count and first + count <= tok_off[b + 1]
        if good:
            d, detail = fit_span(v[first: first + count], lock[first: first + count], int(span_frames[s]))
            res["details"][s] = detail
            good = d is not None
            if good:
                dur[first: first + count] = d
                res["scale"][s] = detail["scale"]
        res["ok"] = res["ok"] and good
    return res


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 2, 3, 63, 64, 65, 1000, 4096)
KINDS = ("n", "n+1", "sum", "50n")


def _case(name, v, tok_lens, spans, targets, lock=None, max_count=None, void=None, structural=False, range_bad=False):
    tok_off = np.concatenate([[0], np.cumsum(tok_lens)]).astype(np.int32)
    spans = np.asarray(spans, np.int32).reshape(-1, 2)
    return dict(name=name, v=np.asarray(v, np.float32), tok_off=tok_off, span_tok=spans, span_frames=np.asarray(targets, np.int32),
                lock=None if lock is None else np.asarray(lock, np.int32),
                max_count=int(max_count if max_count is not None else max(1, min(MAX_COUNT, int(spans[:, 1].max())))),
                void=sorted(void or []), structural=structural, range_bad=range_bad)


def _durations(rng, n):
    return np.exp(rng.normal(1.0, 0.8, n)).astype(np.float32).clip(0.05, 60.0)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case; every case is seeded by its place in this list"""
    out = []
    for count in COUNTS:
        for kind in KINDS:
            rng = np.random.default_rng(1000 + 10 * count + KINDS.index(kind))
            v = _durations(rng, count + 5)                   # the span is the middle utterance: tokens outside every span on both sides
            r = sum(plain(x) for x in v[2: 2 + count])
            T = {"n": count, "n+1": count + 1, "sum": r + int(rng.integers(-3, 4)) if count > 3 else r, "50n": 50 * count}[kind]
            out.append(_case(f"count{count}_{kind}", v, [2, count, 3], [(2, count)], [max(T, count)]))
    out.append(_case("equal_weights", np.full(37, 2.5, np.float32), [37], [(0, 37)], [37 * 3 + 5]))
    out.append(_case("huge_and_tiny", [16000.0] + [0.01] * 60 + [0.02] * 39, [100], [(0, 100)], [150]))
    rng = np.random.default_rng(7)
    v = _durations(rng, 20)
    out.append(_case("all_locked", v, [20], [(0, 20)], [sum(plain(x) for x in v)], lock=[1] * 20))
    v = _durations(rng, 48)
    lock = (rng.random(48) < 0.3).astype(np.int32)
    out.append(_case("hold_some", v, [48], [(4, 40)], [3 * sum(plain(x) for x in v[4:44])], lock=lock))
    v = _durations(rng, 50)
    out.append(_case("adjacent_spans", v, [50], [(0, 10), (10, 15), (25, 25)], [40, 15, 200]))
    v = _durations(rng, 90)
    out.append(_case("several_utterances", v, [30, 0, 25, 35], [(0, 30), (32, 10), (55, 35)], [100, 33, 1000]))
    v = _durations(rng, 1200)
    spans = [(4 * i, 3 + (i % 2)) for i in range(300)]
    out.append(_case("spans300", v, [400, 800], spans, [int(t) for t in rng.integers(4, 80, 300)]))
    # ---- void: structural defects void every span
    v = _durations(rng, 40)
    out.append(_case("void_overlap", v, [40], [(0, 10), (9, 5)], [30, 20], structural=True, void=[0, 1]))
    out.append(_case("void_negative_first", v, [40], [(-1, 5), (10, 5)], [30, 20], structural=True, void=[0, 1]))
    out.append(_case("void_empty_span", v, [40], [(0, 5), (10, 0)], [30, 20], max_count=8, structural=True, void=[0, 1]))
    out.append(_case("void_past_the_end", v, [40], [(0, 5), (36, 5)], [30, 20], structural=True, void=[0, 1]))
    out.append(_case("void_out_of_order", v, [40], [(20, 5), (0, 5)], [30, 20], structural=True, void=[0, 1]))
    # ---- void: one span only
    out.append(_case("void_count_above_max", v, [40], [(0, 5), (10, 9), (30, 5)], [30, 40, 20], max_count=8, void=[1]))
    out.append(_case("void_across_utterances", v, [12, 28], [(0, 5), (10, 5), (30, 5)], [30, 40, 20], void=[1]))
    out.append(_case("void_all_locked_other_sum", v, [40], [(0, 5), (10, 5)], [30, 1 + sum(plain(x) for x in v[10:15])],
                     lock=[0] * 10 + [1] * 5 + [0] * 25, void=[1]))
    out.append(_case("void_target_below_count", v, [40], [(0, 5), (10, 5), (20, 5)], [4, 5, 0], void=[0, 2]))
    out.append(_case("void_negative_target", v, [40], [(0, 5), (10, 5)], [-7, 25], void=[0]))
    out.append(_case("void_above_16384", v, [40], [(0, 2), (10, 5)], [40000, 25], void=[0]))
    out.append(_case("void_target_beyond_any", v, [40], [(0, 5), (10, 5)], [2 ** 30, 25], void=[0]))
    w = v.copy()
    w[[3, 12, 33]] = [np.inf, np.nan, -np.inf]
    out.append(_case("not_finite", w, [40], [(0, 5), (10, 5)], [30, 25], range_bad=True))
    return {c["name"]: c for c in out}


@functools.lru_cache(maxsize=None)
def expected(name):
    c = cases()[name]
    return fit(c["v"], [int(x) for x in c["tok_off"]], [(int(a), int(b)) for a, b in c["span_tok"]], c["span_frames"], c["lock"], c["max_count"])
