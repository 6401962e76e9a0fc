"""HiFi-GAN generator on the HIP path -- SURVEY.md section 8(f) row N2, the step right after the acoustic model
(test.py:115: ``self.generator(mel_rec)``).  Mirrors ``Vocoder/vocoder.py:75-125``: ``Generator(h)``,
``load_state_dict`` (weight-norm folded), ``forward(mel [B, 80, T]) -> wav [B, 1, 300 T]``.

Everything dense runs through the conv GEMM of the acoustic path (``ops.conv_gemm``, bf16x6 arithmetic):
  conv_pre / conv_post   k = 7 convs (LeakyReLU(0.01) and tanh fused around conv_post)
  ResBlock1              18 dilated convs per stage, LeakyReLU(0.1) fused on the input operand, residual in the epilogue
  ConvTranspose1d(2u, u) ONE 3-tap conv with u x Cout output rows (phase, channel) + ``interleave_phases``:
                         out[u q + r] = sum_j w[:, :, (r+p)%u + u j] x[q + (r+p)//u - j]  (p = padding), i.e. taps
                         x[q-1], x[q], x[q+1] with a per-phase weight (zero where a phase does not use the tap)
Activations stay in the packed-frames layout, so a ragged batch costs nothing and every utterance equals its B = 1 result.

``Generator(h, runtime=True)`` runs the same launch sequence inside the library (``as_vocoder_forward``, csrc/vocoder_rt.hip): one C call
per batch instead of ~110, capturable into a graph, with the samples as 16-bit PCM from the last kernel on request.  The default is the
operator-by-operator sequence below.
"""
import ctypes

import numpy as np
import torch

from . import _lib, ops, stage
from .ops import ACT_LRELU, ACT_NONE, ACT_TANH, layout, taps_1d
from .synth import hash_tensor
from .weights import fold_state_dict

LRELU_SLOPE = 0.1                      # vocoder.py:8

DEFAULT_H = dict(resblock="1", upsample_rates=[10, 5, 3, 2], upsample_kernel_sizes=[20, 10, 6, 4],
                 upsample_initial_channel=512, resblock_kernel_sizes=[3, 7, 11],
                 resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_mels=80)    # Vocoder/config.json


def generator_spec(h=None):
    """name -> shape of the reference Generator's state dict (weight-norm parametrisation, vocoder.py:75-99)."""
    h = {**DEFAULT_H, **(h or {})}
    c0, spec = h["upsample_initial_channel"], {}

    def wn(name, shape, g_len):
        spec[name + ".bias"] = (shape[1] if name.startswith("ups.") else shape[0],)
        spec[name + ".weight_g"] = (g_len, 1, 1)
        spec[name + ".weight_v"] = tuple(shape)

    wn("conv_pre", (c0, h["num_mels"], 7), c0)
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        cin, cout = c0 // 2 ** i, c0 // 2 ** (i + 1)
        wn(f"ups.{i}", (cin, cout, k), cin)               # ConvTranspose1d weight [Cin, Cout, k]; weight_norm over dim 0
    n = 0
    for i in range(len(h["upsample_rates"])):
        ch = c0 // 2 ** (i + 1)
        for k, dil in zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"]):
            for j in range(len(dil)):
                wn(f"resblocks.{n}.convs1.{j}", (ch, ch, k), ch)
            for j in range(len(dil)):
                wn(f"resblocks.{n}.convs2.{j}", (ch, ch, k), ch)
            n += 1
    wn("conv_post", (1, c0 // 2 ** len(h["upsample_rates"]), 7), 1)
    return spec


def synth_generator_state_dict(h=None, seed=3407):
    """Seeded synthetic Generator checkpoint (no vocoder weights ship with the reference: README.md:52 is a link).
    Directions U(+-1/sqrt(fan_in)), gains chosen so that activations stay O(1) through the 4 x 18 residual convs."""
    sd = {}
    for name, shape in generator_spec(h).items():
        if name.endswith(".weight_v"):
            # conv [Cout, Cin, k]: fan-in Cin * k; ConvTranspose1d [Cin, Cout, 2u]: two taps reach an output sample
            fan = shape[0] * 2 if name.startswith("ups.") else shape[1] * shape[2]
            sd[name] = hash_tensor("voc." + name, shape, seed, 1.0 / np.sqrt(fan))
        elif name.endswith(".weight_g"):
            sd[name] = None                                 # filled below (needs ||v||)
        else:
            sd[name] = hash_tensor("voc." + name, shape, seed, 0.05)
    for name in list(sd):
        if name.endswith(".weight_g"):
            v = sd[name[:-len("weight_g")] + "weight_v"]
            norm = np.sqrt((v.reshape(v.shape[0], -1).astype(np.float64) ** 2).sum(1)).astype(np.float32).reshape(-1, 1, 1)
            gain = 0.6 if ".convs" in name else 1.0          # residual branches damped
            jitter = 1.0 + 0.1 * hash_tensor("voc." + name, (v.shape[0], 1, 1), seed, 1.0)
            sd[name] = (norm * np.float32(gain) * jitter).astype(np.float32)
    return sd


def _dil_taps(k, d):
    return [(0, d * (t - k // 2)) for t in range(k)]


class Generator:
    """``Generator(h)`` of Vocoder/vocoder.py:75-125 (ResBlock1 configuration)."""

    def __init__(self, h=None, device=None, runtime=False):
        self.h = {**DEFAULT_H, **(h if isinstance(h, dict) else (vars(h) if h is not None else {}))}
        if str(self.h["resblock"]) != "1":
            raise NotImplementedError("only the ResBlock1 generator of Vocoder/config.json is built")
        from .models import _need_gpu
        self.device = _need_gpu(device if device is not None else "cuda")
        self.W = None
        self.runtime = bool(runtime)
        self._voc = self._plan = self._ws = self._ws_cap = self._ws_win = None
        self.halo = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _release(self):
        L = _lib.lib()
        if self._plan:
            torch.cuda.synchronize(self.device)
            L.as_plan_destroy(self._plan)
        if self._voc:
            L.as_vocoder_destroy(self._voc)
        self._voc = self._plan = self._ws = self._ws_cap = self._ws_win = None

    # ------------------------------------------------------------------ the library's generator (runtime=True)
    def runtime_cfg(self):
        """the as_vocoder_cfg of self.h"""
        h, c = self.h, _lib.VocoderCfg()
        rates, ks, rk, rd = h["upsample_rates"], h["upsample_kernel_sizes"], h["resblock_kernel_sizes"], h["resblock_dilation_sizes"]
        if len(rates) > 8 or len(rk) > 4 or any(len(d) != len(rd[0]) or len(d) > 4 for d in rd) or len(rk) != len(rd) or len(ks) != len(rates):
            raise NotImplementedError("as_vocoder_cfg holds up to 8 stages and 4 stacks of up to 4 dilations each")
        c.num_mels, c.upsample_initial_channel, c.n_stages, c.n_stacks, c.n_dilations = h["num_mels"], h["upsample_initial_channel"], len(rates), len(rk), len(rd[0])
        for i, (u, k) in enumerate(zip(rates, ks)):
            c.upsample_rates[i], c.upsample_kernel_sizes[i] = u, k
        for j, (k, dil) in enumerate(zip(rk, rd)):
            c.resblock_kernel_sizes[j] = k
            for n, d in enumerate(dil):
                c.resblock_dilations[j][n] = d
        return c

    def _load_runtime(self, sd):
        """as_vocoder_create on the state dict.  The blob holds the weights as fold_state_dict folds them (plain ``weight`` keys, which the
        library takes as they are -- a checkpoint saved after remove_weight_norm() looks the same): torch's fp32 norm and the library's
        own weight_norm fold (a float64 sum, what a C host gets from a weight_g / weight_v blob) differ in the last bit of about a third
        of the weights, and the two Python paths are meant to agree bit for bit.  Everything else -- the ConvTranspose1d -> phase conv
        rewrite, per-row biases, the fp32 conv_post row, the weight images -- happens in the library."""
        from .blob import state_dict_to_blob
        self._release()
        blob = state_dict_to_blob(fold_state_dict(sd))
        cfg, voc, plan = self.runtime_cfg(), ctypes.c_void_p(), ctypes.c_void_p()
        L = _lib.lib()
        with torch.cuda.device(self.device):
            _lib.check(L.as_vocoder_create(blob, len(blob), ctypes.byref(cfg), ctypes.byref(voc)), "as_vocoder_create")
            self._voc = voc
            _lib.check(L.as_vocoder_plan_create(voc, ctypes.byref(plan)), "as_vocoder_plan_create")
            self._plan = plan
        self.hop = L.as_vocoder_hop(voc)
        self.halo = L.as_vocoder_halo(voc)                 # mel frames a window needs on either side (csrc/window_rule.h)
        return self

    def _library_call(self, what, fn, slot, plan, mel_p, wav, pcm, lay=None, off=None, mult=0, cap=0, max_len=0, out=None):
        """The one call into the library's generator behind forward_packed (runtime=True), forward_packed_cap and forward_packed_windowed:
        the checks, as_vocoder_io (and as_vocoder_cap), the outputs (or out=) and the workspace -> (wav, sample_off or None, pcm).
        fn: the library's function; slot: the attribute that keeps ITS workspace, which only ever grows; plan(B), asked after the checks ->
        (the bytes fn needs, the error text for 0 bytes, the geometry fn takes in front of its io -- None: the as_vocoder_cap of off, mult,
        cap, max_len -- and what it takes between the io and the workspace).  lay: host widths (as_vocoder_forward) instead of a capacity."""
        if not self.runtime:
            raise ValueError(f"{what} needs Generator(runtime=True)")
        if self._voc is None:
            raise RuntimeError("no weights loaded: call load_state_dict first")
        if not (wav or pcm):
            raise ValueError(f"{what}: at least one of wav and pcm")
        r = stage.Device(self.device)
        B = lay.B if lay is not None else r.need(off, stage.I32, what, "off").numel() - 1
        with torch.cuda.device(self.device):
            need, bad, geometry, extra = plan(B)
            if need == 0:
                raise _lib.HipLibraryError(bad)
            ws = getattr(self, slot)
            if ws is None or ws.numel() < need:
                ws = torch.empty(need, dtype=torch.uint8, device=self.device)
                setattr(self, slot, ws)
            if out is not None:
                out_w, sample_off, out_p = out
            else:
                out_w, out_p = stage.samples(r, cap * self.hop if lay is None else max(lay.N * self.hop, 1), wav, pcm, what, lead=(1,))
                sample_off = r.empty(B + 1, stage.I32) if lay is None else None
            io = _lib.VocoderIO(mel=ops._p(mel_p), ld_mel=ops._ld(mel_p), wav=ops._p(out_w), pcm=ops._p(out_p))
            if geometry is None:
                geometry = ctypes.byref(_lib.VocoderCap(off=off.data_ptr(), mult=int(mult), cap=cap, max_len=max_len, sample_off=sample_off.data_ptr()))
            _lib.check(fn(self._voc, self._plan, B, geometry, ctypes.byref(io), *extra, ws.data_ptr(), ws.numel(), _lib.stream()), fn.__name__)
        return out_w, sample_off, out_p

    def _forward_runtime(self, mel_p, lay, wav=True, pcm=False):
        """as_vocoder_forward on the current stream.  The workspace is kept and only ever grows: a graph captured from this generator
        stays valid as long as no larger geometry has been run since."""
        L = _lib.lib()
        lens = (ctypes.c_int32 * lay.B)(*lay.widths_host)
        bad = "as_vocoder_workspace_bytes: invalid geometry (an utterance beyond AS_META_MAX_W samples?)"
        out_w, _, out_p = self._library_call("forward_packed", L.as_vocoder_forward, "_ws", lambda B: (
            L.as_vocoder_workspace_bytes(self._voc, self._plan, B, lens), bad, lens, ()), mel_p, wav, pcm, lay=lay)
        lay_w = lay.scaled(self.hop)
        return (out_w, lay_w, out_p) if pcm else (out_w, lay_w)

    def forward_packed_cap(self, mel_p, off, mult, cap, max_len=None, pcm=False, wav=True):
        """The generator when the frame counts exist on the device only (as_vocoder_forward_cap; runtime=True): mel_p [80][>= cap] packed
        from column 0, `off` a DEVICE int32 [B + 1] in units of `mult` mel frames (a forward_packed(frame_cap=)'s frame_off: mult = 2),
        `cap` mel frames of room for all utterances together, max_len the frames one utterance may have (None: cap).  No host value is
        read, nothing synchronises: the call can be captured with whatever produced `off` and `mel_p`.  Returns (wav [1][300 cap] or None,
        sample_off device int32 [B + 1]) and, with pcm=True, the int16 samples [300 cap]: utterance b is [sample_off[b], sample_off[b + 1]),
        the samples behind the last utterance are 0.  More frames than room raises the AS_STATUS_CAPACITY bit (as_device_status)."""
        L = _lib.lib()
        cap, max_len = int(cap), int(max_len or 0)
        bad = "as_vocoder_cap_workspace_bytes: invalid capacity (max_len > cap, or an utterance beyond AS_META_MAX_W samples?)"
        res = self._library_call("forward_packed_cap", L.as_vocoder_forward_cap, "_ws_cap", lambda B: (
            L.as_vocoder_cap_workspace_bytes(self._voc, self._plan, B, cap, max_len), bad, None, ()), mel_p, wav, pcm, None, off, mult, cap, max_len)
        return res if pcm else res[:2]

    def forward_packed_windowed(self, mel_p, off, mult, cap, core, max_len=None, halo=None, pcm=False, wav=True, rounds=None, out=None):
        """forward_packed_cap in rounds of `core` mel frames per utterance (as_vocoder_forward_windowed; csrc/window_rule.h): the same
        arguments, the same return value and output layout, the same samples within the module's bound -- every round vocodes each
        utterance's next `core` frames with `halo` frames of context on either side (None: self.halo, the generator's receptive field) and
        stores the core's samples in place.  The workspace is this method's own, depends on B, core and halo only (not on cap) and only ever
        grows: a graph captured from this call stays valid as long as no larger (B, core, halo) has been run since.
        rounds = (round0, n): only those rounds (n = 0: every round from round0 on); round 0 also writes the filler's zeros and sample_off.
        out = (wav, sample_off, pcm) of an earlier call: the buffers to write into (rounds in pieces)."""
        L = _lib.lib()

        def window(B):                              # (after the checks: without weights there is no hop)
            wc = _lib.WindowCfg(int(core), -1 if halo is None else int(halo), self.hop)
            round0, n_rounds = (0, 0) if rounds is None else (int(rounds[0]), int(rounds[1]))
            if round0 < 0 or n_rounds < 0:
                raise ValueError("forward_packed_windowed: rounds = (first round >= 0, count >= 0)")
            return (L.as_vocoder_windowed_workspace_bytes(self._voc, self._plan, B, ctypes.byref(wc)),
                    "as_vocoder_windowed_workspace_bytes: invalid window (core < 1, halo < -1, or a window beyond AS_META_MAX_W samples?)",
                    None, (ctypes.byref(wc), round0, n_rounds))

        res = self._library_call("forward_packed_windowed", L.as_vocoder_forward_windowed, "_ws_win", window, mel_p, wav, pcm, None, off, mult,
                                 int(cap), int(max_len or 0), out)
        return res if pcm else res[:2]

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd, strict=False):
        sd = sd.get("generator", sd) if isinstance(sd, dict) else sd       # test.py:124: checkpoint['generator']
        if self.runtime:
            return self._load_runtime(sd)
        w = fold_state_dict(sd)
        dev, h, W = self.device, self.h, {}
        W["pre"] = (ops.prep_weight(w["conv_pre.weight"], dev), w["conv_pre.bias"].to(dev))
        W["post"] = (ops.prep_weight(w["conv_post.weight"], dev), w["conv_post.bias"].to(dev))
        wp = w["conv_post.weight"]                                           # [1][C][7]: one output row -- plain FMAs (ops.conv_post)
        W["post32"] = wp[0].float().contiguous().to(dev) if wp.shape[0] == 1 and wp.shape[2] in (3, 5, 7) else None
        for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
            if k != 2 * u:
                raise NotImplementedError("ConvTranspose1d with k != 2 * stride")
            wt = w[f"ups.{i}.weight"]                                      # [Cin, Cout, k]
            cin, cout = wt.shape[0], wt.shape[1]
            p = u // 2 + u % 2
            wc = torch.zeros(u * cout, cin, 3)                             # rows (phase r', channel m); taps dw = -1, 0, +1
            for r in range(u):
                rr, s = (r + p) % u, (r + p) // u
                for j in (0, 1):
                    dw = s - j
                    wc[r * cout:(r + 1) * cout, :, dw + 1] = wt[:, :, rr + u * j].t()
            W[f"ups{i}"] = (ops.prep_weight(wc, dev), w[f"ups.{i}.bias"].to(dev), u, cout)
            W[f"ups{i}b"] = w[f"ups.{i}.bias"].repeat(u).to(dev)               # per row (phase, channel): the interleaved store adds it
        n = 0
        for i in range(len(h["upsample_rates"])):
            for k, dil in zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"]):
                blk = []
                for j, d in enumerate(dil):
                    blk.append((ops.prep_weight(w[f"resblocks.{n}.convs1.{j}.weight"], dev), w[f"resblocks.{n}.convs1.{j}.bias"].to(dev),
                                _dil_taps(k, d),
                                ops.prep_weight(w[f"resblocks.{n}.convs2.{j}.weight"], dev), w[f"resblocks.{n}.convs2.{j}.bias"].to(dev),
                                _dil_taps(k, 1)))
                W[f"rb{n}"] = blk
                n += 1
        self.W = W
        return self

    def remove_weight_norm(self):                                          # folded at load
        return self

    def eval(self):
        return self

    def to(self, device):
        return self

    # ------------------------------------------------------------------ forward
    def forward_packed(self, mel_p, lay, pcm=False, wav=True):
        """mel_p [80][sum T] packed -> (wav [1][300 sum T], layout of the samples); pcm=True: also the samples as int16 [300 sum T],
        converted by the last kernel (as_conv_post_pcm_f32's rule); wav=False (runtime=True, with pcm): no fp32 samples are written (None)."""
        if self.runtime:
            with torch.cuda.device(self.device):
                return self._forward_runtime(mel_p, lay, wav=wav, pcm=pcm)
        if not wav:
            raise ValueError("forward_packed(wav=False) needs Generator(runtime=True)")
        W, h = self.W, self.h
        if W is None:
            raise RuntimeError("no weights loaded: call load_state_dict first")
        wt, b = W["pre"]
        x = ops.conv_gemm(wt, mel_p, lay, lay.new(wt.shape[2]), taps_1d(7), bias=b)
        nk = len(h["resblock_kernel_sizes"])
        nst = len(h["upsample_rates"])
        xi = None                                   # LeakyReLU(x) as an operand image, when the producer of x wrote that instead of x
        for i in range(nst):
            wt, b, u, cout = W[f"ups{i}"]
            lay_up = lay.scaled(u)
            # ConvTranspose1d as one 3-tap conv with (phase, channel) rows: its epilogue stores the rows in time order (ileave) -- the
            # interleave_phases pass over the stage's input is gone -- when the channels are a multiple of 32
            il = cout % 32 == 0
            out = lay_up.new(cout) if il else lay.new(u * cout)
            kw = dict(bias=W[f"ups{i}b"], ileave=u) if il else {}
            if xi is not None:
                z = ops.conv_gemm(wt, None, lay, out, taps_1d(3), xs=xi, K=h["upsample_initial_channel"] // 2 ** i, **kw)
                xi = None
            else:
                z = ops.conv_gemm(wt, x, lay, out, taps_1d(3), in_act=ACT_LRELU, in_slope=LRELU_SLOPE, **kw)
            # 32 / 64 channels: the residual steps are fused launches (below); they address a tensor with 32-bit byte offsets: a batch
            # beyond 2 GiB per tensor takes the conv GEMM launches.  (Reading the conv's phase-major output in place -- the interleave as an
            # address computation of their six reads, ops.respair's (Z, bias, u) form -- was measured: 14.30 ms per batch against 14.08 with
            # the interleave kernel: the six strided reads cost more than the 0.28 ms the two passes take.)
            fused = cout in (32, 64) and nk == 3 and 4 * u * cout * (lay.N + 1) < 2 ** 31
            x = z if il else ops.interleave_phases(z, b, cout, u, lay.N, lay_up.new(cout))
            lay = lay_up
            outs = []
            # LeakyReLU(x) as an operand image, once for the three residual stacks that start from x; inside a stack every conv hands its
            # LeakyReLU'd result to the next one as an image (ConvGemmArgs.Yh / yh_lrelu): no fp32 copy of conv1's output, no split passes
            # (the three stacks of a stage as ONE launch per step -- ops.conv_gemm_multi -- was measured: 18.2 ms per batch against 17.9 with
            # a launch per conv; these grids hold thousands of tiles each, there is no tail worth filling)
            if fused:
                # 32 / 64 channels: a residual step is ONE launch that keeps its column tile in LDS between the two convs (ops.respair):
                # x in, y out -- no operand images in HBM at all; the stage's mean rides in the last step of the third stack
                for j in range(nk):
                    y = x
                    blk = W[f"rb{i * nk + j}"]
                    for n, (w1, b1, t1, w2, b2, t2) in enumerate(blk):
                        last = j + 1 == nk and n + 1 == len(blk)
                        # (the stage's mean feeds only the next ConvTranspose1d: its last step writes LeakyReLU(mean) as that conv's image)
                        y = ops.respair(y, lay, w1, b1, w2, b2, len(t1), t1[1][1] - t1[0][1] if len(t1) > 1 else 1, LRELU_SLOPE,
                                        add=(outs[0], outs[1]) if last else None,
                                        image_slope=LRELU_SLOPE if last and i + 1 < nst else None)
                    outs.append(y)
                if i + 1 < nst:
                    x, xi = None, outs[2]
                else:
                    x = outs[2]
                continue
            xh = ops.split_act(x, lay, in_act=ACT_LRELU, in_slope=LRELU_SLOPE)
            for j in range(nk):
                y, yh = x, xh
                blk = W[f"rb{i * nk + j}"]
                for n, (w1, b1, t1, w2, b2, t2) in enumerate(blk):
                    xth = ops.new_image(cout, lay.N, x.device)
                    ops.conv_gemm(w1, None, lay, None, t1, bias=b1, xs=yh, K=cout, yh=xth, yh_lrelu=True, in_slope=LRELU_SLOPE)
                    last = n + 1 == len(blk)
                    yh = None if last else ops.new_image(cout, lay.N, x.device)
                    y = ops.conv_gemm(w2, None, lay, lay.new(cout), t2, bias=b2, res=y, xs=xth, K=cout, yh=yh, yh_lrelu=not last,
                                      in_slope=LRELU_SLOPE)
                outs.append(y)
            if nk != 3:
                raise NotImplementedError("three residual stacks per stage (Vocoder/config.json)")
            if i + 1 < nst:
                x, xi = None, ops.mean3_image(outs[0], outs[1], outs[2], lay.N, LRELU_SLOPE)
            else:
                x = ops.mean3(outs[0], outs[1], outs[2], lay.N, lay.new(cout))
        wt, b = W["post"]
        if pcm:
            if W["post32"] is None:
                raise NotImplementedError("16-bit samples from the operator-level path need the fp32 conv_post kernel (k = 3, 5, 7)")
            wav, p16 = ops.conv_post(x, lay, W["post32"], b, 0.01, pcm=True)
            return wav, lay, p16
        if W["post32"] is not None:
            wav = ops.conv_post(x, lay, W["post32"], b, 0.01)
        else:
            wav = ops.conv_gemm(wt, x, lay, lay.new(1), taps_1d(7), bias=b, in_act=ACT_LRELU, in_slope=0.01, act=ACT_TANH)
        return wav, lay

    @torch.no_grad()
    def forward(self, x, lengths=None, pcm16=False):
        """x: mel [B, 80, T] (zero-padded beyond `lengths`) -> wav [B, 1, 300 * T], zero beyond each utterance; pcm16=True: the same as
        int16 samples converted on the device (forward_packed(pcm=True))."""
        from .models import pack, unpack
        B, _, T = x.shape
        lens = [int(v) for v in lengths] if lengths is not None else [T] * B
        lay = layout(lens, self.device)
        with torch.cuda.device(self.device):
            if pcm16:
                _, lay_w, p16 = self.forward_packed(pack(x.to(self.device), lens), lay, pcm=True)
                return unpack(p16[None], lay_w)
            wav, lay_w = self.forward_packed(pack(x.to(self.device), lens), lay)
        return unpack(wav, lay_w)

    __call__ = forward
