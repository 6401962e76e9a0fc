"""CPU: the checkpoint side of the C runtime as artspeech_amd/csrc/checkpoint.h states it, without a GPU: the "ASWBLOB1" reader on
well-formed and on malformed blobs, the weight_norm / spectral_norm fold, the twin-tower merge and every host assembly as_model's
getters and as_vocoder_create upload.  The header is plain C++17: the probe beside this file (checkpoint_probe.cpp, compiled here with
g++, once plain and once under AddressSanitizer + UBSan) hands blobs to its functions and writes the resulting tensors to a file.

The expected values are never the header's: they are numpy restatements written here (bit for bit: the assemblies are copies, zero
fills and single fp32 additions; the folds' sums are SEQUENTIAL float64 additions of products of two fp32 numbers, which are exact in
float64, so neither fusing nor the compiler changes a bit), artspeech_amd/blob.py for the format, and the lines of
artspeech_amd/vocoder.py::Generator.load_state_dict that build `wc` and `ups{i}b` for the generator."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from artspeech_amd import _lib, synth
from artspeech_amd import vocoder as V
from artspeech_amd.blob import state_dict_to_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": [], "sanitized": ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------------------------
# the probe
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(BUILDS))
def probe(request, tmp_path_factory):
    """`sanitized`: the same stand-alone program under AddressSanitizer and UBSan (a finding ends it with a non-zero status)"""
    d = tmp_path_factory.mktemp("checkpoint_probe_" + request.param)
    exe = d / "checkpoint_probe"
    subprocess.check_call(["g++", "-std=c++17", *BUILDS[request.param], "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "tests", "checkpoint_probe.cpp"), "-o", str(exe)])
    src, out, last = d / "in.bin", d / "out.bin", [None]

    def run(op, blob, *args):
        """-> (the lines printed, name -> array of what the probe wrote)"""
        if blob is not last[0]:
            src.write_bytes(blob)
            last[0] = blob
        if out.exists():
            out.unlink()
        lines = subprocess.check_output([str(exe), op, str(src), str(out), *[str(a) for a in args]], text=True).splitlines()
        return lines, parse_dump(out.read_bytes()) if out.exists() else {}

    return run


def parse_dump(b):
    got, o = {}, 0
    while o < len(b):
        nl, = struct.unpack_from("<I", b, o)
        name = b[o + 4: o + 4 + nl].decode()
        o += 4 + nl
        nd, = struct.unpack_from("<I", b, o)
        dims = struct.unpack_from(f"<{nd}i", b, o + 4)
        n, = struct.unpack_from("<Q", b, o + 4 + 4 * nd)
        o += 12 + 4 * nd
        assert name not in got and n == int(np.prod(dims, dtype=np.int64)), (name, dims, n)
        got[name] = np.frombuffer(b[o: o + 4 * n], "<f4").reshape(dims)
        o += 4 * n
    return got


def same(a, b):
    """the same shape and the same bits"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == f32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same_maps(got, want):
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert same(got[k], v), k
    return True


# ------------------------------------------------------------------------------------------------------------------------------------
# the checkpoints
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_sd():
    return synth.synth_state_dict(64, 8, seed=11)


@pytest.fixture(scope="module")
def model_folded(model_sd):
    return fold_np(model_sd)


TINY_H = dict(V.DEFAULT_H, upsample_initial_channel=32)


@pytest.fixture(scope="module")
def generator_sd():
    return V.synth_generator_state_dict(TINY_H, seed=3407)


def small_sd():
    g = np.random.default_rng(5)
    return {"a": g.standard_normal((2, 3)).astype(f32), "bb.weight": g.standard_normal(4).astype(f32), "c": np.array([1.5], f32)}


def raw_blob(entries, data, magic=b"ASWBLOB1", count=None, data_bytes=None):
    """The format of artspeech_amd/blob.py from raw fields, so that a field can lie.  entries: (name bytes, dims, data_offset) with
    optional overrides {"name_len": , "ndim": } as a fourth element."""
    b = magic + struct.pack("<I", len(entries) if count is None else count)
    for e in entries:
        name, dims, off = e[:3]
        lie = e[3] if len(e) > 3 else {}
        b += struct.pack("<H", lie.get("name_len", len(name))) + name + struct.pack("<B", lie.get("ndim", len(dims)))
        b += struct.pack(f"<{len(dims)}I", *dims) + struct.pack("<Q", off)
    return b + struct.pack("<Q", len(data) if data_bytes is None else data_bytes) + data


def small_parts():
    sd = small_sd()
    data = sd["a"].tobytes() + b"\0" * 8 + sd["bb.weight"].tobytes() + sd["c"].tobytes() + b"\0" * 12
    return [(b"a", (2, 3), 0), (b"bb.weight", (4,), 32), (b"c", (1,), 48)], data


def malformed():
    """label -> blob: every one has to be refused"""
    ents, data = small_parts()
    small = raw_blob(ents, data)
    assert small == state_dict_to_blob(small_sd()) and len(small) < 300
    bad = {f"prefix {n}": small[:n] for n in range(len(small))}
    bad["bytes given as 11"] = small[:11]
    bad["wrong magic"] = b"NOTABLOB" + small[8:]
    bad["count 0xFFFFFFFF"] = raw_blob(ents, data, count=0xFFFFFFFF)
    bad["count one more than fits"] = raw_blob(ents, data, count=(len(small) - 12) // 11 + 1)
    bad["name_len 0xFFFF"] = raw_blob([(b"a", (2, 3), 0, {"name_len": 0xFFFF})] + ents[1:], data)
    for nd in (9, 255):
        bad[f"ndim {nd}"] = raw_blob([(b"a", (2, 3), 0, {"ndim": nd})] + ents[1:], data)
    bad["ndim 9 with its dims"] = raw_blob([(b"a", (1,) * 9, 0)] + ents[1:], data)
    bad["dim above INT32_MAX"] = raw_blob([(b"a", (2, 0x80000000), 0)] + ents[1:], data)
    bad["4 numel wraps to 0"] = raw_blob([(b"a", (1 << 30, 1 << 30, 4), 0)] + ents[1:], data)
    bad["numel wraps"] = raw_blob([(b"a", (0x7FFFFFFF,) * 8, 0)] + ents[1:], data)
    bad["data_offset beyond data_bytes"] = raw_blob(ents[:2] + [(b"c", (1,), len(data) + 1)], data)
    bad["end one past data_bytes"] = raw_blob(ents[:2] + [(b"c", (1,), len(data) - 3)], data)
    bad["data_bytes one more than is left"] = raw_blob(ents, data, data_bytes=len(data) + 1)
    return small, bad


# ------------------------------------------------------------------------------------------------------------------------------------
# numpy restatements
# ------------------------------------------------------------------------------------------------------------------------------------
def seq_sum(p):
    """sum over the last axis of float64 `p` by sequential addition (np.sum adds pairwise)"""
    return np.add.accumulate(p, axis=-1)[..., -1]


def fold_np(sd):
    """The fold: weight_norm  scale = g / float32(sqrt(sum v^2)), w = v * scale in fp32;  spectral_norm  s_r = float32(sum_i W[r, i] v[i]),
    sigma = sum_r float64(u[r]) * float64(s_r), w = W / float32(sigma); every sum sequential in float64.  Names: `module.` stripped, the
    two extractors dropped, weight_v / weight_u not passed on."""
    sd = {(k[7:] if k.startswith("module.") else k): np.asarray(v, f32) for k, v in sd.items()}
    out = {}
    for k, t in sd.items():
        if k.startswith(("style_encoder.pitch_extractor.", "style_encoder.ema_extractor.")):
            continue
        if k.endswith(".weight_g"):
            v = sd[k[:-9] + ".weight_v"]
            v2 = v.reshape(v.shape[0], -1)
            s = seq_sum(v2.astype(f64) * v2.astype(f64))
            scale = t.reshape(-1) / np.sqrt(s).astype(f32)
            assert scale.dtype == f32
            out[k[:-9] + ".weight"] = (v2 * scale[:, None]).reshape(v.shape)
        elif k.endswith(".weight_orig"):
            u, v = sd[k[:-12] + ".weight_u"], sd[k[:-12] + ".weight_v"]
            w2 = t.reshape(t.shape[0], -1)
            s = seq_sum(w2.astype(f64) * v.astype(f64)[None, :]).astype(f32)
            sigma = seq_sum(u.astype(f64) * s.astype(f64))
            out[k[:-12] + ".weight"] = t / f32(sigma)
        elif not k.endswith((".weight_v", ".weight_u")):
            out[k] = t
    assert all(v.dtype == f32 for v in out.values())
    return out


def block_diag(a, b):
    co, ci = a.shape[:2]
    t = np.zeros((2 * co, 2 * ci) + a.shape[2:], f32)
    t[:co, :ci], t[co:, ci:] = a, b
    return t


def mat(got):
    return got["w"], got["w2"], got["b"]


# ------------------------------------------------------------------------------------------------------------------------------------
# the reader
# ------------------------------------------------------------------------------------------------------------------------------------
def test_reader_round_trips_the_synthetic_checkpoints(probe, model_sd, generator_sd):
    for sd in (model_sd, generator_sd, small_sd()):
        lines, got = probe("read", state_dict_to_blob(sd))
        assert lines == ["ok"] and same_maps(got, {k: np.asarray(v, f32) for k, v in sd.items()})


def test_reader_on_hand_made_entries(probe):
    g = np.random.default_rng(7)
    x8 = g.standard_normal((1, 2, 1, 3, 1, 2, 1, 2)).astype(f32)
    first, later = g.standard_normal(3).astype(f32), g.standard_normal((2, 2)).astype(f32)
    data = np.array(2.5, f32).tobytes() + x8.tobytes() + first.tobytes() + later.tobytes()
    o8, o1, o2 = 4, 4 + x8.nbytes, 4 + x8.nbytes + 12
    ents = [(b"scalar", (), 0), (b"none", (3, 0, 2), len(data)), (b"eight", x8.shape, o8), (b"", (3,), o1), (b"twice", (3,), o1),
            (b"twice", (2, 2), o2)]
    lines, got = probe("read", raw_blob(ents, data))
    assert lines == ["ok"]
    assert same_maps(got, {"scalar": np.array(2.5, f32), "none": np.zeros((3, 0, 2), f32), "eight": x8, "": first, "twice": later})
    lines, got = probe("read", raw_blob([], b""))                         # zero entries
    assert lines == ["ok"] and got == {}
    assert probe("read", state_dict_to_blob({}))[0] == ["ok"]


def test_reader_refuses_malformed_blobs(probe):
    small, bad = malformed()
    records = b"".join(struct.pack("<Q", len(b)) + b for b in [small, *bad.values()])
    lines, _ = probe("reject", records)
    assert lines[0] == "1"                                               # (the blob the cases were cut from is read)
    assert dict(zip(bad, lines[1:])) == {k: "0" for k in bad} and len(lines) == 1 + len(bad)


def _tiny_vocoder_cfg():
    cfg = _lib.VocoderCfg()
    cfg.num_mels, cfg.upsample_initial_channel, cfg.n_stages, cfg.n_stacks, cfg.n_dilations = 80, 32, 4, 3, 3
    for i, (u, k) in enumerate(zip(TINY_H["upsample_rates"], TINY_H["upsample_kernel_sizes"])):
        cfg.upsample_rates[i], cfg.upsample_kernel_sizes[i] = u, k
    for j, (k, dil) in enumerate(zip(TINY_H["resblock_kernel_sizes"], TINY_H["resblock_dilation_sizes"])):
        cfg.resblock_kernel_sizes[j] = k
        for n, d in enumerate(dil):
            cfg.resblock_dilations[j][n] = d
    return cfg


def test_library_refuses_malformed_blobs_without_a_device():
    """The same blobs through as_model_create and as_vocoder_create of the built library: AS_EINVAL on a machine without a GPU, because
    the reader runs before a device is asked for anything."""
    L = _lib.lib()
    small, bad = malformed()
    mcfg = _lib.ModelCfg()
    mcfg.hidden_dim, mcfg.dim_in, mcfg.style_dim, mcfg.n_mels, mcfg.n_token = 64, 8, 256, 80, 178
    vcfg, out = _tiny_vocoder_cfg(), ctypes.c_void_p()
    cases = [(k, b, len(b)) for k, b in bad.items()] + [("full blob, bytes given as 11", small, 11)]
    for label, b, n in cases:
        assert L.as_model_create(b, n, ctypes.byref(mcfg), ctypes.byref(out)) == -1, label
        assert L.as_vocoder_create(b, n, ctypes.byref(vcfg), ctypes.byref(out)) == -1, label
    assert not out.value


# ------------------------------------------------------------------------------------------------------------------------------------
# the folds
# ------------------------------------------------------------------------------------------------------------------------------------
def test_fold_bit_for_bit(probe, model_sd, model_folded, generator_sd):
    lines, got = probe("fold", state_dict_to_blob(model_sd))
    assert lines == ["ok"] and same_maps(got, model_folded)
    assert not [k for k in got if k.endswith((".weight_v", ".weight_u", ".weight_g", ".weight_orig"))]
    lines, got = probe("fold", state_dict_to_blob(generator_sd))
    assert lines == ["ok"] and same_maps(got, fold_np(generator_sd))


def test_fold_names_and_missing_parts(probe):
    g = np.random.default_rng(9)
    r = lambda *s: g.standard_normal(s).astype(f32)
    sd = {"module.a.weight_g": r(4, 1, 1), "module.a.weight_v": r(4, 3, 2), "module.a.bias": r(4),
          "b.weight_orig": r(5, 2, 3), "b.weight_u": r(5), "b.weight_v": r(6), "module.plain": r(2, 2),
          "style_encoder.pitch_extractor.conv.weight": r(3), "module.style_encoder.ema_extractor.fc.bias": r(3)}
    ents, data, off = [], b"", 0                       # (blob.py strips `module.` and drops the extractors itself: written raw here)
    for k, v in sd.items():
        ents.append((k.encode(), v.shape, off))
        data += v.tobytes()
        off += v.nbytes
    lines, got = probe("fold", raw_blob(ents, data))
    assert lines == ["ok"] and sorted(got) == ["a.bias", "a.weight", "b.weight", "plain"]
    assert same_maps(got, fold_np(sd))
    for drop in ("module.a.weight_v", "b.weight_u", "b.weight_v"):
        assert probe("fold", raw_blob([e for e in ents if e[0].decode() != drop], data))[0] == ["fail fold"], drop
    for k, v in (("module.a.weight_g", r(3, 1, 1)), ("b.weight_u", r(4)), ("b.weight_v", r(5))):      # a part of the wrong length
        wrong = dict(sd)
        wrong[k] = v
        ents2, data2, off = [], b"", 0
        for kk, vv in wrong.items():
            ents2.append((kk.encode(), vv.shape, off))
            data2 += vv.tobytes()
            off += vv.nbytes
        assert probe("fold", raw_blob(ents2, data2))[0] == ["fail fold"], k


# ------------------------------------------------------------------------------------------------------------------------------------
# the twins
# ------------------------------------------------------------------------------------------------------------------------------------
def test_twin_towers_and_linears(probe, model_sd, model_folded):
    blob = state_dict_to_blob(model_sd)
    a, b, m = "style_encoder.energy_block", "style_encoder.F0_block", "style_encoder.ENF0_block"
    want = dict(model_folded)                                             # the originals remain
    for k, ta in model_folded.items():
        if not k.startswith(a + "."):
            continue
        tb = model_folded[b + k[len(a):]]
        cat = not k.endswith(".weight") or ".pool." in k
        want[m + k[len(a):]] = np.concatenate([ta, tb]) if cat else block_diag(ta, tb)
    assert len(want) > len(model_folded) + 20 and want[m + ".1.pool.weight"].shape == (16, 1, 3)
    lines, got = probe("towers", blob, a, b, m)
    assert lines == ["ok"] and same_maps(got, want)

    la, lb, lm = "style_encoder.Energylinear", "style_encoder.F0linear", "style_encoder.ENF0linear"
    wa, wb = model_folded[la + ".weight"], model_folded[lb + ".weight"]
    o, i = wa.shape
    w = np.zeros((2 * o, 2 * i), f32)
    w[:o, i:], w[o:, :i] = wb, wa                                         # [lb on the second input half | la on the first]
    want = dict(model_folded)
    want[lm + ".weight"], want[lm + ".bias"] = w, np.concatenate([model_folded[lb + ".bias"], model_folded[la + ".bias"]])
    lines, got = probe("linears", blob, la, lb, lm)
    assert lines == ["ok"] and same_maps(got, want)

    # shapes that do not match, a twin that is not there
    g = np.random.default_rng(2)
    r = lambda *s: g.standard_normal(s).astype(f32)
    odd = {"a.0.weight": r(4, 2, 3), "a.0.bias": r(4), "b.0.weight": r(4, 3, 3), "b.0.bias": r(4),
           "la.weight": r(4, 6), "la.bias": r(4), "lb.weight": r(4, 5), "lb.bias": r(4)}
    assert probe("towers", state_dict_to_blob(odd), "a", "b", "m")[0] == ["fail merge_twin_towers"]
    assert probe("towers", state_dict_to_blob(odd), "none", "b", "m")[0] == ["fail merge_twin_towers"]
    assert probe("linears", state_dict_to_blob(odd), "la", "lb", "m")[0] == ["fail merge_twin_linears"]
    del odd["b.0.bias"], odd["lb.bias"]
    assert probe("towers", state_dict_to_blob(odd), "a", "b", "m")[0] == ["fail merge_twin_towers"]
    assert probe("linears", state_dict_to_blob(odd), "la", "lb", "m")[0] == ["fail merge_twin_linears"]


# ------------------------------------------------------------------------------------------------------------------------------------
# the acoustic model's assemblies
# ------------------------------------------------------------------------------------------------------------------------------------
def without(sd, *names):
    """the checkpoint without what folds to `names` (a weight-normed tensor: its g and v)"""
    drop = set()
    for n in names:
        drop |= {n, n + "_g", n + "_v", n + "_orig", n + "_u"}
    return state_dict_to_blob({k: v for k, v in sd.items() if k not in drop})


USED = ("attn_layers.0.conv_", "attn_layers.1.conv_", "LSTM.", ".norm1.fc.", "_conv.", "dur_block.", "artsPredictor.F0.", "artsPredictor.N.",
        "Mel_block.0.")


def test_assemblies_bit_for_bit(probe, model_sd, model_folded):
    """(on the part of the checkpoint that the calls below name: the probe reads and folds its blob on every call)"""
    model_sd = {k: v for k, v in model_sd.items() if any(u in k for u in USED)}
    blob, F = state_dict_to_blob(model_sd), model_folded
    cat = lambda names: np.concatenate([F[n].reshape(-1) for n in names])

    # q / k / v: one prefix, two
    te, ae = "text_encoder.encoder.attn_layers.0", "arts_encoder.encoder.attn_layers.1"
    for ps in ([te], [te, ae]):
        lines, got = probe("qkv", blob, *ps)
        w, w2, b = mat(got)
        assert lines == ["ok"] and w.shape == (len(ps), 192, 64, 1) and w2.size == 0
        assert same(w.reshape(-1), cat([f"{p}.conv_{n}.weight" for p in ps for n in "qkv"]))
        assert same(b, cat([f"{p}.conv_{n}.bias" for p in ps for n in "qkv"]))
    assert probe("qkv", without(model_sd, ae + ".conv_k.bias"), te, ae)[0] == [f"fail {ae}.conv_k.bias"]
    assert probe("qkv", without(model_sd, ae + ".conv_v.weight", ae + ".conv_v.bias"), te, ae)[0] == [f"fail {ae}.conv_v.weight"]

    # the LSTM input projection: one name, three
    three = [f"artsPredictor.{n}_LSTM" for n in ("F0", "N", "EMA")]
    for names in (["durationPredictor.LSTM"], three):
        lines, got = probe("lstm_wih", blob, *names)
        w, w2, b = mat(got)
        H, I = F[names[0] + ".weight_hh_l0"].shape[1], F[names[0] + ".weight_ih_l0"].shape[1]
        assert lines == ["ok"] and w.shape == (len(names), 8 * H, I, 1)
        assert same(w.reshape(-1), cat([f"{p}.weight_ih_l0{d}" for p in names for d in ("", "_reverse")]))
        assert same(b, np.concatenate([F[f"{p}.bias_ih_l0{d}"] + F[f"{p}.bias_hh_l0{d}"] for p in names for d in ("", "_reverse")]))
    assert probe("lstm_wih", without(model_sd, three[1] + ".bias_hh_l0"), *three)[0] == [f"fail {three[1]}.bias_hh_l0"]

    # W_hh transposed
    p = "durationPredictor.LSTM"
    lines, got = probe("lstm_whh_t", blob, p)
    assert lines == ["ok"] and same(got["t"], np.stack([F[p + ".weight_hh_l0"].T, F[p + ".weight_hh_l0_reverse"].T]))
    assert got["t"].shape == (2, 32, 128)
    assert probe("lstm_whh_t", without(model_sd, p + ".weight_hh_l0_reverse"), p)[0] == [f"fail {p}.weight_hh_l0_reverse"]

    # fc_all: slices of the 512 style entries, two of them behind the start
    norms = [("artsPredictor.shared.norm1", 0, 512), ("artsPredictor.F0.1.norm1", 128, 64), ("artsPredictor.EMA.2.norm1", 384, 128),
             ("decoder.decode.3.norm1", 256, 256), ("artsPredictor.N.2.norm1", 0, 64)]
    spec = [f"{n}:{off}:{S}" for n, off, S in norms]
    lines, got = probe("fc_all", blob, 512, *spec)
    w, w2, b = mat(got)
    want, row0, at = [], [], 0
    for n, off, S in norms:
        wt = F[n + ".fc.weight"]
        z = np.zeros((wt.shape[0], 512), f32)
        z[:, off:off + S] = wt
        want.append(z)
        row0.append(f"{n} {at}")
        at += wt.shape[0]
    assert lines == ["ok"] + row0 and at == 128 + 128 + 64 + 128 + 64
    assert w.shape == (1, at, 512, 1) and same(w.reshape(at, 512), np.concatenate(want)) and same(b, cat([n + ".fc.bias" for n, _, _ in norms]))
    assert probe("fc_all", without(model_sd, norms[2][0] + ".fc.bias"), 512, *spec)[0] == [f"fail {norms[2][0]}.fc.bias"]
    assert probe("fc_all", blob, 512, spec[0], "artsPredictor.F0.1.norm1:128:32")[0] == ["fail "]          # S is not the layer's
    assert probe("fc_all", blob, 512, spec[0], "artsPredictor.F0.1.norm1:449:64")[0] == ["fail "]          # the slice ends behind K

    # fne: block diagonal [128][12]
    lines, got = probe("fne", blob)
    w, w2, b = mat(got)
    want = np.zeros((128, 12), f32)
    want[:32, 0], want[32:64, 1] = F["decoder.F0_conv.weight"].reshape(32), F["decoder.N_conv.weight"].reshape(32)
    want[64:, 2:] = F["decoder.EMA_conv.weight"].reshape(64, 10)
    assert lines == ["ok"] and w.shape == (1, 128, 12, 1) and same(w.reshape(128, 12), want)
    assert same(b, cat([f"decoder.{n}_conv.bias" for n in ("F0", "N", "EMA")]))
    assert probe("fne", without(model_sd, "decoder.N_conv.bias"))[0] == ["fail decoder.N_conv.bias"]
    assert probe("fne", without(model_sd, "decoder.EMA_conv.weight", "decoder.F0_conv.bias"))[0] == ["fail decoder.EMA_conv.weight"]

    # conv_stack of two, conv_fold of two; the plain concatenation
    c1 = ["durationPredictor.dur_block.2.conv1", "durationPredictor.dur_block.3.conv1"]
    lines, got = probe("conv_stack", blob, *c1)
    w, w2, b = mat(got)
    assert lines == ["ok"] and w.shape == (2, 128, 128, 9) and same(w.reshape(-1), cat([n + ".weight" for n in c1])) and w2.size == b.size == 0
    assert probe("conv_stack", without(model_sd, c1[1] + ".weight"), *c1)[0] == [f"fail {c1[1]}.weight"]
    assert probe("conv_stack", blob, c1[0], "durationPredictor.dur_block.1.conv1")[0] == ["fail "]         # another shape
    c2, sc = [f"artsPredictor.{n}.1.conv2" for n in ("F0", "N")], [f"artsPredictor.{n}.1.conv1x1" for n in ("F0", "N")]
    lines, got = probe("conv_fold", blob, ",".join(c2), ",".join(sc))
    w, w2, b = mat(got)
    Cout, Cin, T = F[c2[0] + ".weight"].shape
    assert lines == ["ok"] and w.shape == (2, Cout, Cin, T) and w2.shape == (2, 32, 64) and Cout == 32
    assert same(w.reshape(-1), cat([n + ".weight" for n in c2])) and same(w2.reshape(-1), cat([n + ".weight" for n in sc]))
    assert probe("conv_fold", without(model_sd, sc[1] + ".weight"), ",".join(c2), ",".join(sc))[0] == [f"fail {sc[1]}.weight"]
    assert probe("conv_fold", blob, ",".join(c2), sc[0])[0] == ["fail "]                                   # one shortcut for two convs
    assert probe("conv_fold", blob, ",".join(c2), sc[0] + ",artsPredictor.F0.2.conv1x1")[0] == ["fail "]   # a shortcut of another shape
    v2 = ["durationPredictor.LSTM.bias_ih_l0", "durationPredictor.LSTM.bias_hh_l0_reverse"]
    lines, got = probe("concat", blob, 0, *v2)
    assert lines == ["ok"] and same(got["v"], cat(v2))
    assert probe("concat", blob, 0, v2[0], "no.such.tensor")[0] == ["fail no.such.tensor"]
    assert probe("concat", blob, 0, v2[0], "artsPredictor.F0_LSTM.bias_ih_l0")[0] == ["fail "]             # another length

    # the direct kernel's image of a Cin = 1 weight: [T][Kp][M], only row 0 of the 16 filled
    n = "style_encoder.Mel_block.0.weight"
    lines, got = probe("direct_image", blob, n, 16)
    want = np.zeros((9, 16, 8), f32)
    want[:, 0, :] = F[n].reshape(8, 9).T
    assert lines == ["ok"] and same(got["w32"], want)


# ------------------------------------------------------------------------------------------------------------------------------------
# the generator's checkpoint
# ------------------------------------------------------------------------------------------------------------------------------------
def test_generator_assemblies(probe, generator_sd):
    """checkpoint_ok on the tiny generator, and the ConvTranspose1d -> phase conv fold with its row bias for u = 10, 5, 3, 2 (the four
    stages) against the construction of Generator.load_state_dict (vocoder.py: `wc`, `ups{i}b`), in numpy."""
    blob, F = state_dict_to_blob(generator_sd), fold_np(generator_sd)
    shape = [80, 32, 4, 3, 3, 16, *TINY_H["upsample_kernel_sizes"], *TINY_H["resblock_kernel_sizes"]]
    assert probe("generator_ok", blob, *shape)[0] == ["ok"]
    assert probe("generator_ok", without(generator_sd, "ups.2.bias"), *shape)[0] == ["fail vocoder checkpoint has no tensor 'ups.2.bias'"]
    assert probe("generator_ok", without(generator_sd, "conv_post.weight"), *shape)[0] == \
        ["fail vocoder checkpoint has no tensor 'conv_post.weight'"]
    wide = list(shape)
    wide[1] = 64
    assert probe("generator_ok", blob, *wide)[0] == ["fail vocoder tensor 'conv_pre.weight' has another shape"]
    k5 = list(shape)
    k5[10] = 5                                                           # the first stack's kernel size
    assert probe("generator_ok", blob, *k5)[0] == ["fail vocoder tensor 'resblocks.0.convs1.0.weight' has another shape"]
    few = list(shape)
    few[5] = 5                                                           # conv_post has 7 taps
    assert probe("generator_ok", blob, *few)[0] == ["fail vocoder tensor 'conv_post.weight' has another shape"]
    for i, u in enumerate(TINY_H["upsample_rates"]):
        wt, bias = F[f"ups.{i}.weight"], F[f"ups.{i}.bias"]             # [Cin, Cout, 2u]
        cin, cout = wt.shape[:2]
        p = u // 2 + u % 2
        wc = np.zeros((u * cout, cin, 3), f32)
        for r in range(u):
            rr, s = (r + p) % u, (r + p) // u
            for j in (0, 1):
                dw = s - j
                wc[r * cout:(r + 1) * cout, :, dw + 1] = wt[:, :, rr + u * j].T
        lines, got = probe("upsample", blob, f"ups.{i}", u)
        assert lines == ["ok"] and same(got["wc"], wc) and same(got["rows"], np.tile(bias, u)), (i, u)
    assert {10, 5, 3, 2} == set(TINY_H["upsample_rates"])
