"""The entries of spec_models.py whose libraries ``__graft_entry__.build()`` compiles a second time WITHOUT the forced
include of mjpl_amd/csrc/mjpl_overlay.h, under spec/plain/ -- tests/test_gpu_overlay.py compares the two builds.
One per slot-file kind: the benchmark model (eight wide), a random tree four wide, one sixteen wide (the overlay leaves
that width to the compiler's indexed moves) and the model with moving boxes (literal slots: SpecSlots)."""
from spec_models import spec_models

PLAIN_SUBDIR = "plain"

# name prefix in spec_models() -> (slot-file width the program must have, moving boxes)
OVERLAY_CASES = (("franka_p+16obs, arm planned", 8, False),
                 ("random_model(1005)", 4, False),
                 ("random_model(1002)", 16, False),
                 ("franka_p+16obs+10 pad boxes", 24, True))


def overlay_models():
    """[(entry of spec_models(), width, moving boxes)] in the order of OVERLAY_CASES."""
    entries = spec_models()
    out = []
    for prefix, width, mbox in OVERLAY_CASES:
        found = [e for e in entries if e[0].startswith(prefix)]
        assert len(found) == 1, prefix
        out.append((found[0], width, mbox))
    return out
