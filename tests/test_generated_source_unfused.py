"""The two switches of the fused pose text (specialise.Options.pose_fma / .sincos, mjpl_pose_f32.h).  Off -- the
generator's own default, and what tests/test_generated_source.py holds against the recorded digests -- the text has
no call of a helper in it; build() generates with pose_fma on (Options.for_build) unless the environment says 0 -- sincos is an opt-in -- and a
translation unit includes mjpl_pose_f32.h exactly when its text calls a helper.  The header is not a stamped one: the
program hash and the stamp do not depend on it.  And the text build() does generate is pinned like the default one:
tests/golden/generated_source_digests_build.json (tools/make_generated_digests.py: compute_build) holds the digest of
every model's generated check and of every translation unit __graft_entry__.build() compiles, under Options.for_build().
Host only: no GPU, no compiler."""
import json

import pytest

from mjpl_amd import build as build_mod
from mjpl_amd import specialise as sp
from spec_models import spec_models

from test_generated_source import tool

COMBOS = ((True, True), (True, False), (False, True), (False, False))


@pytest.fixture(scope="module")
def bench():
    name, model, allowed, qidx, base = spec_models()[0]
    return model, allowed, qidx, base


def test_each_switch_alone_changes_the_text_and_off_is_the_default(bench, monkeypatch):
    for var in ("MJPL_SPEC_POSE_FMA", "MJPL_SPEC_SINCOS"):
        monkeypatch.delenv(var, raising=False)
    ip, fp, dp, info = sp.dump_program(*bench)
    texts = {o: sp.generate(ip, fp, dp, info, opts=sp.Options(pose_fma=o[0], sincos=o[1])) for o in COMBOS}
    assert len(set(texts.values())) == 4
    assert "sincosf(" not in texts[(True, True)] and "sincos_half_f32(" not in texts[(True, False)]
    assert "mjpl::pose_" in texts[(True, False)] and "__builtin_fmaf(-nq3, sn, nq0 * cs)" in texts[(True, True)]
    assert "mjpl::pose_" not in texts[(False, True)] and "mjpl::pose_" not in texts[(False, False)]
    assert sp.generate(ip, fp, dp, info) == texts[(False, False)]  # (the recorded text: test_generated_source.py)
    assert sp.Options() == sp.Options.from_env()
    assert (sp.Options.for_build().pose_fma, sp.Options.for_build().sincos) == (True, False)
    monkeypatch.setenv("MJPL_SPEC_SINCOS", "1")
    monkeypatch.setenv("MJPL_SPEC_POSE_FMA", "0")
    assert (sp.Options.for_build().pose_fma, sp.Options.for_build().sincos) == (False, True)


def test_a_unit_includes_the_header_exactly_when_its_text_calls_a_helper(bench):
    include = '#include "mjpl_pose_f32.h"'
    for o in COMBOS:
        key, src = sp.library_source(*bench, opts=sp.Options(pose_fma=o[0], sincos=o[1]))
        assert (include in src) == (o[0] or o[1]), o
        assert (("mjpl::pose_" in src) or ("mjpl::sincos_half_f32" in src)) == (o[0] or o[1]), o
    assert key == int(sp.dump_program(*bench)[3].hash)  # (one hash for all four: the comparison libraries need an `output`)
    assert "mjpl_pose_f32.h" not in build_mod.STAMPED_HEADERS


def test_build_generates_the_fused_text_unless_told_otherwise(bench, monkeypatch):
    """specialise.build()'s source, by its compile line's input: the text hipcc would be given."""
    seen = []

    class Done(Exception):
        pass

    def record(src, *a, **kw):
        seen.append(src)
        raise Done

    monkeypatch.setattr(sp, "_compile", record)
    for var in ("MJPL_SPEC_POSE_FMA", "MJPL_SPEC_SINCOS"):
        monkeypatch.delenv(var, raising=False)
    with pytest.raises(Done):
        sp.build(*bench, force=True)
    with pytest.raises(Done):
        sp.build(*bench, force=True, opts=sp.Options.for_build()._replace(pose_fma=False, sincos=False))
    assert "mjpl::pose_quat2mat" in seen[0] and "mjpl_pose_f32.h" in seen[0] and "sincosf(" in seen[0]  # (sincos: opt-in)
    assert "mjpl::pose_" not in seen[1] and "sincos_half_f32" not in seen[1] and "mjpl_pose_f32.h" not in seen[1]


def test_every_text_build_generates_equals_the_recorded_one():
    with open(tool.BUILD_GOLDEN) as f:
        golden = json.load(f)
    with open(tool.GOLDEN) as f:
        plain = json.load(f)
    with pytest.MonkeyPatch.context() as mp:
        computed = tool.compute_build(mp)
    assert sorted(computed["models"]) == sorted(golden["models"]) == sorted(plain["models"])
    for model, want in golden["models"].items():
        got = computed["models"][model]
        assert got["hash"] == want["hash"] == plain["models"][model]["hash"], model
        wrong = [k for k in want if got.get(k) != want[k]]
        assert sorted(got) == sorted(want) and not wrong, f"{model}: build() generates another text for: {'; '.join(wrong)}"
        assert want["spec"] != plain["models"][model]["spec"], model
    assert sum(w["spec"] != w["spec, sincos"] for w in golden["models"].values()) >= 9  # (every model with a hinge)
    assert sorted(computed["translation units"]) == sorted(golden["translation units"]) == sorted(plain["translation units"])
    wrong = [k for k, v in golden["translation units"].items() if computed["translation units"][k] != v]
    assert not wrong, f"build() composes another translation unit for: {'; '.join(wrong)}"
    assert not set(golden["translation units"].values()) & set(plain["translation units"].values())
