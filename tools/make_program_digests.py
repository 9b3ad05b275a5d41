"""tests/golden/program_digests.json: sha256 of the program tables (ip, fp, dp) of the models tests/test_pair_pruning.py
compiles, with nothing dropped (prune_pairs = 0).  The committed file was recorded from the compiler before it had the
pruning stage; write it again only when the table layout or a constant of these models changes on purpose.
usage: python tools/make_program_digests.py"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mjpl_amd import specialise  # noqa: E402
from spec_models import spec_models  # noqa: E402


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    out = {}
    for name, model, allowed, qidx, base in spec_models():
        if name.startswith(("franka_p+16obs, arm planned", "ur5e", "random_model", "two_dof_ball")):
            ip, fp, dp = specialise.dump_program_pruned(model, allowed, qidx, base, prune_pairs=0)[:3]
            out[name.split(" (")[0]] = {"ip": digest(ip), "fp": digest(fp), "dp": digest(dp)}
    with open(os.path.join(ROOT, "tests", "golden", "program_digests.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(sorted(out), indent=1))


if __name__ == "__main__":
    main()
