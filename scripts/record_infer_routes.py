#!/usr/bin/env python3
"""Record what se3tn_infer launches: for every configuration of CASES in tests/test_gpu_routes.py and every n = 1 .. 72, the launch
names of one profiled call and the stages se3tn_debug_buffer hands out afterwards -> tests/golden/infer_routes.json (runs of identical
consecutive n are stored once: [first n, last n, names, stages]).  One process; the first error ends it.

    python scripts/record_infer_routes.py [OUT.json]

The file is a record of the commit it was taken at (tests/golden/PROVENANCE.txt): tests/test_host_abi.py holds the host-side plan
(csrc/infer_plan.h) against it, cell by cell."""
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # test_gpu_routes imports its route model (tests/route_model.py) by name
import se3tracknet_amd as se3
from oracle import se3_oracle as O

N_MAX = 72


def main(out_path):
    import test_gpu_routes as T
    ref = {"sd": O.make_state_dict(21)}
    g = torch.Generator().manual_seed(5)
    A = (0.1 * torch.randn((N_MAX, 4, 176, 176), generator=g)).cuda()
    B = (0.1 * torch.randn((N_MAX, 4, 176, 176), generator=g)).cuda()
    cases = []
    for case in T.CASES:
        eng, cfg = T._engine(se3, ref, case["env"], case["ops"], N_MAX)
        rows = []
        try:
            for n in range(1, N_MAX + 1):
                eng.profile_enable(1)
                try:
                    eng.infer(A, B, n, se3.NCHW)
                    names = [nm for nm, _ in eng.profile_launches(0)]
                finally:
                    eng.profile_enable(0)
                torch.cuda.synchronize()
                stages = [s for s, t in T._readable(se3, eng, n).items() if t is not None]
                if rows and rows[-1][2] == names and rows[-1][3] == stages:
                    rows[-1][1] = n
                else:
                    rows.append([n, n, names, stages])
        finally:
            eng.close()
        cases.append({"id": case["id"], "env": case["env"], "ops": [list(op) for op in case["ops"]], "cfg": cfg, "rows": rows})
        print("%-28s %d runs of n" % (case["id"], len(rows)), flush=True)
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = None
    with open(out_path, "w") as f:
        json.dump({"commit": commit, "n_max": N_MAX, "cases": cases}, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "infer_routes.json"))
