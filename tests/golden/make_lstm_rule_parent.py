"""Records lstm_rule_parent.json beside this file: what as_bilstm_plan and as_bilstm_cluster_bytes of the library AS BUILT IN THIS TREE
answer over the grid below.  Meant to be run once, on a checkout of the commit whose answers are to be kept (no GPU needed: both are host
functions), with that commit's id as the argument:

    python tests/golden/make_lstm_rule_parent.py <commit>

The plans are stored as runs [value, count] over itertools.product(mode, n_jobs, B, H, max_len, buffer), the last index fastest.
buffer: "absent" = no exchange buffer, "exact" = one of as_bilstm_cluster_bytes(n_jobs, B) bytes, "short" = one byte less (never below
0).  mode: AS_LSTM_CLUSTER in the environment, null = unset."""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

GRID = {
    "mode": [None, "0", "1", "2", "3"],
    "n_jobs": [0, 1, 2, 3, 4, 5],
    "B": [-1, 0, 1, 2, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 85, 86, 128, 256, 257],
    "H": [-16, 0, 8, 16, 24, 32, 48, 64, 80, 96, 128, 240, 256, 272],
    "max_len": [0, 1, 40, (1 << 17) - 1, 1 << 17],
    "buffer": ["absent", "exact", "short"],
}


def main(commit):
    from artspeech_amd import _lib
    L = _lib.lib()
    nbytes = [[int(L.as_bilstm_cluster_bytes(j, b)) for b in GRID["B"]] for j in GRID["n_jobs"]]
    runs = []
    for mode, j, b, h, ml, buf in itertools.product(*GRID.values()):
        if mode is None:
            os.environ.pop("AS_LSTM_CLUSTER", None)
        else:
            os.environ["AS_LSTM_CLUSTER"] = mode
        exact = nbytes[GRID["n_jobs"].index(j)][GRID["B"].index(b)]
        p = int(L.as_bilstm_plan(j, b, h, ml, int(buf != "absent"), {"absent": 0, "exact": exact, "short": max(exact - 1, 0)}[buf]))
        if runs and runs[-1][0] == p:
            runs[-1][1] += 1
        else:
            runs.append([p, 1])
    with open(os.path.join(HERE, "lstm_rule_parent.json"), "w") as f:
        json.dump({"parent": commit, "grid": GRID, "cluster_bytes": nbytes, "plan_runs": runs}, f, separators=(",", ":"))
        f.write("\n")
    print(sum(n for _, n in runs), "plans in", len(runs), "runs")


if __name__ == "__main__":
    main(sys.argv[1])
