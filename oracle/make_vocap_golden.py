"""Runs the REFERENCE's own eval_ycb.VOCap on seeded error arrays and stores what it computes in tests/golden/vocap_reference.npz
(TEST INFRASTRUCTURE ONLY; needs the reference tree, see oracle/ref_shims.py):

    python -m oracle.make_vocap_golden [out_dir]

  errs [20, 200]  float64, np.random.default_rng(0).exponential(0.03, 200) twenty times
  tied [20, 200]  np.round(errs, 2): many exact ties, some exactly 0 and exactly 0.1
  vocap_errs / vocap_tied [20]  eval_ycb.VOCap of each row"""
import importlib.util
import os
import sys
import types

import numpy as np

from . import ref_shims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_eval_ycb():
    """eval_ycb.py imported unmodified (pyplot is imported at module level there and never used)"""
    ref_shims.install()
    try:
        import matplotlib.pyplot  # noqa: F401
    except Exception:   # noqa: BLE001
        for m in ("matplotlib", "matplotlib.pyplot"):
            sys.modules.setdefault(m, types.ModuleType(m))
    spec = importlib.util.spec_from_file_location("ref_eval_ycb", os.path.join(ref_shims.REFERENCE_ROOT, "eval_ycb.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    rng = np.random.default_rng(0)
    errs = np.stack([rng.exponential(0.03, 200) for _ in range(20)])
    return errs, np.round(errs, 2)


def run():
    mod = reference_eval_ycb()
    errs, tied = cases()
    return {"errs": errs, "tied": tied,
            "vocap_errs": np.array([mod.VOCap(e) for e in errs], np.float64),
            "vocap_tied": np.array([mod.VOCap(t) for t in tied], np.float64)}


if __name__ == "__main__":
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(out_dir, "vocap_reference.npz"), **run())
