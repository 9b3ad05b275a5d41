"""Host only: mjpl_amd/csrc/mjpl_overlay.h now also specialises the binary32 queue drain, and still changes no layout,
table or value -- so the source stamp and the benchmark program's hash are the recorded ones, the overlay is no stamped
header, and it rides as a forced include on both compile lines (libmjpl_hip.so and the per-model libraries), which
carry no other new option."""
import json
import os

import pytest

from mjpl_amd import build as build_mod
from mjpl_amd import scenes, specialise

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generated_source_digests.json")


def test_stamp_and_benchmark_hash_are_the_recorded_ones():
    """The recorded hash mixes the source stamp in (mjpl_compile.h: mix_stamp): it stands for both."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert f"-DMJPL_SRC_STAMP=0x{build_mod.src_stamp():016x}ull" in build_mod.hipcc_flags()
    m = scenes.franka_p(obstacles=True)
    qidx, base = scenes.planning_index(m, scenes.FRANKA_ARM_JOINTS), m.keyframe("home").qpos.copy()
    info = specialise.dump_program(m, (), qidx, base)[3]
    want = next(v["hash"] for k, v in golden["models"].items() if k.startswith("franka_p+16obs, arm planned"))
    assert f"{int(info.hash):016x}" == want


def test_the_overlay_is_a_forced_include_on_both_lines_and_not_stamped(monkeypatch):
    assert os.path.basename(build_mod.OVERLAY_HEADER) not in build_mod.STAMPED_HEADERS
    with open(build_mod.OVERLAY_HEADER) as f:
        text = f.read()
    assert "queue_drain<float, BOXQ, ALL, false>" in text and "slot_get6<float, 8>" in text
    assert not any("overlay" in f for f in build_mod.hipcc_flags())  # (the stamp's line is what it was)
    assert build_mod.codegen_flags() == ["-mllvm", "-structurizecfg-skip-uniform-regions"]
    lines = []

    class Done(Exception):
        pass

    def record(cmd, **kw):
        lines.append(list(cmd))
        raise Done

    monkeypatch.setattr(build_mod.subprocess, "run", record)
    monkeypatch.setattr(specialise.subprocess, "run", record)
    with pytest.raises(Done):
        build_mod.build_hip(force=True)
    scratch = os.path.join(specialise.SPEC_DIR, "overlay_queue_test")
    for overlay in (True, False):
        with pytest.raises(Done):
            specialise._compile("", scratch + ".hip", scratch + ".so", False, (), overlay=overlay)
    assert not [f for f in os.listdir(specialise.SPEC_DIR) if f.startswith("overlay_queue_test")]
    hip, spec_on, spec_off = lines
    for line in (hip, spec_on):
        at = line.index("-include")
        assert os.path.samefile(line[at + 1], build_mod.OVERLAY_HEADER)
        assert line.count("-include") == 1
    assert "-include" not in spec_off
    assert [f for f in spec_on if f not in spec_off] == ["-include", build_mod.OVERLAY_HEADER]
    # nothing on the lines but the base flags, the stamp, the overlay and codegen_flags() (and, per model, its own fixed ones)
    known = set(build_mod.hipcc_flags()) | set(build_mod.overlay_flags()) | set(build_mod.codegen_flags())
    assert [f for f in hip[1:-3] if f not in known] == []
