"""One SHA-256 per case of oracle.lstm_ref.FAMILIES over the bytes that the recurrence kernels write: every case goes through ops.bilstm as
tests/test_lstm_bound_gpu.py launches it (padded gx, padded or shared outputs, AS_LSTM_CLUSTER as the case says, a fresh exchange buffer
for the cluster cases).  Two builds that compute the same bits print the same lines; needs only artspeech_amd.ops and oracle/lstm_ref.py,
so it runs unchanged on an older checkout."""
import hashlib
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from artspeech_amd import ops
from oracle import lstm_ref as R

dev = torch.device("cuda:0")
for family in sorted(R.FAMILIES):
    for c in R.FAMILIES[family]():
        if c.mode:
            os.environ["AS_LSTM_CLUSTER"] = c.mode
        else:
            os.environ.pop("AS_LSTM_CLUSTER", None)
        N, H, J = c.N, c.H, c.n_jobs
        gxs = []
        for g in c.gx:
            full = torch.full((N + R.GROWS, 8 * H + (R.GPAD if c.gpad else 0)), float("nan"), device=dev)
            full[:N, :8 * H] = g.to(dev)
            gxs.append(full[:N, :8 * H])
        w = N + (R.OPAD if c.opad else 0)
        buf = torch.full((2 * H, J * w), R.SENTINEL, device=dev)
        if c.shared:
            outs = [buf[:, j * w:j * w + N] for j in range(J)]
        else:
            outs = [torch.full((2 * H, w), R.SENTINEL, device=dev)[:, :N] for _ in range(J)]
        jobs = [(gxs[j], c.whh[j].contiguous().to(dev), outs[j]) for j in range(J)]
        lay = ops.layout(c.lens, dev)
        xchg = ops.bilstm_exchange_buffer(J, c.B, dev) if c.xchg else None
        ops.bilstm(jobs, types.SimpleNamespace(col_off=lay.col_off, B=lay.B, max_w=max(c.lens)), H, xchg)
        torch.cuda.synchronize()
        sha = hashlib.sha256()
        for o in outs:
            sha.update(o.cpu().contiguous().numpy().tobytes())
        print(f"{sha.hexdigest()}  {family} {c.kernel}: {c.describe()}")
