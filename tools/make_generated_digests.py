"""tests/golden/generated_source_digests.json: sha256 of every text mjpl_amd/specialise.py generates for the models of
tests/spec_models.py, and of the translation units library_source() composes, under the generator's own default switches
-- since the fused pose helpers (mjpl_pose_f32.h) that is the text WITHOUT them, which __graft_entry__.build() compiles
under spec/unfused/ only.  tests/golden/generated_source_digests_build.json (compute_build, below) holds the same for
Options.for_build(): the texts and translation units of the libraries build() compiles and engines load.
The generator is host Python over the program tables and deterministic, so a change that is meant to leave the generated
code alone is proved by these digests (tests/test_generated_source.py).  The sha256 of ip / fp / dp and the program
hash are recorded beside them: where THEY differ the compiler's tables changed and the file is to be recorded again;
where only a text differs, the generator changed.

The committed file was recorded at commit c891162 ("Certified edge checks: free bubbles and bisection over whole
edges"), before the generator was split into decoder, analyses and emitters.  Write it again only from a generator whose
output is meant to be the new truth -- never from the code a test is about to judge.  Needs libmjpl_hip.so
(mjpl_program_dump), no GPU and no compiler.
usage: python tools/make_generated_digests.py"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mjpl_amd import specialise as sp  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "generated_source_digests.json")
# ... and of what specialise.build() hands the compiler when its caller passes no switches (Options.for_build(): the fused
# pose arithmetic of mjpl_pose_f32.h) -- the texts of the libraries __graft_entry__.build() compiles; GOLDEN above holds
# the generator's own default, the text without the helpers (tests/test_generated_source_unfused.py compares both)
BUILD_GOLDEN = os.path.join(ROOT, "tests", "golden", "generated_source_digests_build.json")


def sha(x):
    """sha256 of a text or an array; None (a generator that declines) stays None."""
    if x is None:
        return None
    return hashlib.sha256(x.encode() if isinstance(x, str) else np.ascontiguousarray(x).tobytes()).hexdigest()


class ProcessEnv:
    """os.environ behind the two methods of pytest's monkeypatch that `compute` uses."""

    @staticmethod
    def setenv(name, value):
        os.environ[name] = value

    @staticmethod
    def delenv(name, raising=False):
        os.environ.pop(name, None)


def model_digests(entry, env):
    """Every generator output of one spec_models() entry -> {variant: digest}."""
    name, model, allowed, qidx, base = entry
    ip, fp, dp, info = sp.dump_program(model, allowed, qidx, base)
    never = sp.dump_never_touch(model, allowed, qidx, base)[0]
    out = {"ip": sha(ip), "fp": sha(fp), "dp": sha(dp), "hash": f"{int(info.hash):016x}"}
    out["spec"] = sha(sp.generate(ip, fp, dp, info, never_touch=never))
    out["spec, no never-touch set"] = sha(sp.generate(ip, fp, dp, info))
    out["spec, difference culls"] = sha(sp.generate(ip, fp, dp, info, cull_form="difference"))
    if info.scene_ok:
        out["spec, generic"] = sha(sp.generate(ip, fp, dp, info, generic=True))
    env.setenv("MJPL_SPEC_CERT", "1")
    report = {}
    out["spec, MJPL_SPEC_CERT=1"] = sha(sp.generate(ip, fp, dp, info, never_touch=never, report=report))
    out["cert_ok"] = bool(report["cert_ok"])
    env.delenv("MJPL_SPEC_CERT")
    if info.mbox:
        # no committed model makes `generate` fall back to a program without shared box axes: that path by its private name
        out["spec, box axes not shared"] = sha(sp._generate(ip, fp, dp, info, share_axes=False, never_touch=never))
    out["exact"] = sha(sp.generate_exact(ip, dp, info))
    out["exact, generic"] = sha(sp.generate_exact(ip, dp, info, generic=True))
    out["exact, fold=False"] = sha(sp.generate_exact(ip, dp, info, fold=False))
    out["full exact"] = sha(sp.generate_full_exact(ip, fp, dp, info))
    env.setenv("MJPL_SPEC_F64_INLINE", "1")
    out["full exact, MJPL_SPEC_F64_INLINE=1"] = sha(sp.generate_full_exact(ip, fp, dp, info))
    env.delenv("MJPL_SPEC_F64_INLINE")
    out["pose section"] = sha(sp.generate_pose_section(model, int(ip[sp.H_NPLAN]), [int(x) for x in qidx]))
    return out


def library_source(model, allowed, qidx, base, generic=False, prune_contacts=1):
    """The translation unit specialise.build() compiles for these arguments: from the source half of build() where the
    generator has one, else composed here from its public functions the way build() composes it."""
    if hasattr(sp, "library_source"):
        return sp.library_source(model, allowed, qidx, base, generic=generic, prune_contacts=prune_contacts)[1]
    ip, fp, dp, info = sp.dump_program(model, allowed, qidx, base)
    never, _, info.hash, _ = sp.dump_never_touch(model, allowed, qidx, base, prune_contacts=prune_contacts)
    nstage, pc = 0, int(ip[sp.H_OFF_BODYOPS])
    for _ in range(int(ip[sp.H_NBODYOPS])):
        nj, ng = int(ip[pc + sp.B_NJNT]), int(ip[pc + sp.B_NGEOM])
        pc += sp.B_SIZE + nj * sp.J_SIZE + ng * (sp.G_SIZE + sp.MAX_SLOTS)
        nstage += ng
    return sp.translation_unit(
        sp.generate(ip, fp, dp, info, generic=generic, never_touch=never), sp.generate_exact(ip, dp, info, generic=generic),
        info.robot_hash if generic else info.hash, info, (sp.SCENE_ROWS << 8 | nstage) if generic else 0,
        pose=sp.generate_pose_section(model, int(ip[sp.H_NPLAN]), qidx=[int(x) for x in qidx]),
        exact_full=sp.generate_full_exact(ip, fp, dp, info) if (not generic and os.environ.get("MJPL_SPEC_F64") == "1") else None)


def unit_digests(entries, env):
    """The translation units of the libraries __graft_entry__.build() compiles for the benchmark model (the first entry),
    the model with the finger pads (MJPL_SPEC_WAVES, fwaves) and the scene-generic robots."""
    from spec_models import generic_robots
    bench = entries[0][1:]
    pads = next(e for e in entries if "pad boxes" in e[0])[1:]
    out = {"bench": sha(library_source(*bench)), "bench, prune_contacts=0": sha(library_source(*bench, prune_contacts=0))}
    for var in ("MJPL_SPEC_CERT", "MJPL_SPEC_F64"):
        env.setenv(var, "1")
        out[f"bench, {var}=1"] = sha(library_source(*bench))
        env.delenv(var)
    for k, robot in enumerate(generic_robots()):
        out[f"generic robot {k}"] = sha(library_source(*robot, generic=True))
    out["pad boxes"] = sha(library_source(*pads))
    return out


def compute(env):
    """{"models": {entry: {variant: digest}}, "translation units": {library: digest}} with every MJPL_SPEC_* / MJPL_GEN_*
    variable cleared and only what a variant names set, through `env` (setenv / delenv: pytest's monkeypatch, or ProcessEnv)."""
    from spec_models import spec_models
    for name in [n for n in os.environ if n.startswith(("MJPL_SPEC_", "MJPL_GEN_"))]:
        env.delenv(name)
    entries = spec_models()
    return {"models": {e[0]: model_digests(e, env) for e in entries}, "translation units": unit_digests(entries, env)}


def compute_build(env):
    """compute()'s counterpart for Options.for_build(): per model the generated check as build() generates it ("spec",
    "spec, generic") and with the sincos switch on as well ("spec, sincos"); the translation units of unit_digests()."""
    from spec_models import generic_robots, spec_models
    for name in [n for n in os.environ if n.startswith(("MJPL_SPEC_", "MJPL_GEN_"))]:
        env.delenv(name)
    entries = spec_models()
    models = {}
    for name, model, allowed, qidx, base in entries:
        ip, fp, dp, info = sp.dump_program(model, allowed, qidx, base)
        never = sp.dump_never_touch(model, allowed, qidx, base)[0]
        opts = sp.Options.for_build()
        out = {"hash": f"{int(info.hash):016x}", "spec": sha(sp.generate(ip, fp, dp, info, never_touch=never, opts=opts)),
               "spec, sincos": sha(sp.generate(ip, fp, dp, info, never_touch=never, opts=opts._replace(sincos=True)))}
        if info.scene_ok:
            out["spec, generic"] = sha(sp.generate(ip, fp, dp, info, generic=True, opts=opts))
        models[name] = out

    def unit(args, **kw):
        return sha(sp.library_source(*args, opts=sp.Options.for_build(), **kw)[1])

    bench = entries[0][1:]
    units = {"bench": unit(bench), "bench, prune_contacts=0": unit(bench, prune_contacts=0)}
    for var in ("MJPL_SPEC_CERT", "MJPL_SPEC_F64"):
        env.setenv(var, "1")
        units[f"bench, {var}=1"] = unit(bench)
        env.delenv(var)
    for k, robot in enumerate(generic_robots()):
        units[f"generic robot {k}"] = unit(robot, generic=True)
    units["pad boxes"] = unit(next(e for e in entries if "pad boxes" in e[0])[1:])
    return {"models": models, "translation units": units}


def main():
    for path, out in ((GOLDEN, compute(ProcessEnv)), (BUILD_GOLDEN, compute_build(ProcessEnv))):
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps({k: len(v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
