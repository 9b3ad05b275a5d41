"""The generator writes the same text: sha256 of every output of mjpl_amd/specialise.py for the models of spec_models.py,
and of the translation units build() composes, against tests/golden/generated_source_digests.json
(tools/make_generated_digests.py: what is recorded, and from which commit).  Host only: no GPU, no compiler."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_generated_digests", os.path.join(ROOT, "tools", "make_generated_digests.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

TABLES = ("ip", "fp", "dp", "hash")


@pytest.fixture(scope="module")
def golden():
    with open(tool.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def computed():
    with pytest.MonkeyPatch.context() as mp:
        return tool.compute(mp)


def test_every_generated_text_equals_the_recorded_one(golden, computed):
    assert sorted(computed["models"]) == sorted(golden["models"])
    for model, want in golden["models"].items():
        got = computed["models"][model]
        tables = [k for k in TABLES if got[k] != want[k]]
        assert not tables, f"{model}: the program tables differ ({', '.join(tables)}): the compiler changed, record the digests again"
        assert sorted(got) == sorted(want), model
        wrong = [k for k in want if got[k] != want[k]]
        assert not wrong, f"{model}: the generator writes another text for: {'; '.join(wrong)}"


def test_every_translation_unit_equals_the_recorded_one(golden, computed):
    assert sorted(computed["translation units"]) == sorted(golden["translation units"])
    wrong = [k for k, v in golden["translation units"].items() if computed["translation units"][k] != v]
    assert not wrong, f"build() composes another translation unit for: {'; '.join(wrong)}"


def test_the_recorded_variants_cover_the_paths_they_are_there_for(golden):
    """The pad-box model's code without shared box axes is another text, the random moving-box models' is not; the
    certificate is generated into some model's code and refused for another; the float64 check exists for some model."""
    models = golden["models"]
    unshared = {m: v["spec, box axes not shared"] != v["spec"] for m, v in models.items() if "spec, box axes not shared" in v}
    assert len(unshared) == 3 and sum(unshared.values()) == 1 and unshared[next(m for m in models if "pad boxes" in m)]
    assert {v["cert_ok"] for v in models.values()} == {True, False}
    for v in models.values():
        assert (v["spec, MJPL_SPEC_CERT=1"] != v["spec"]) == v["cert_ok"]
        assert v["spec"] != v["spec, difference culls"]
        assert (v["full exact"] is None) == (v["full exact, MJPL_SPEC_F64_INLINE=1"] is None)
    assert any(v["full exact"] is not None for v in models.values())
    units = golden["translation units"]
    assert len(set(units.values())) == len(units) == 7
