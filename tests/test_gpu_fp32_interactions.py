"""GPU (MI355X): one interaction in single precision, every field of its records bounded by the oracle.

The catalogue (tests/fp32_interactions.py): one leaf at coordinates of 30 behind a dense rotation, an aimed fan of 130 rays, the
trace stopped behind the hit.  Every launch that can take the scene — `trace_batch` as called by default, the rolling lists
(OT_OPT_KERNEL = 2), the generations of `Engine.trace_tree` — leaves the same records bit for bit, and those records are the
oracle's: the same records in the same order, `ray` and `surface` equal on EVERY ray the conditioning runs did not exclude (no
0.9995: the fans are clear of every decision), segment 0 the input's bit patterns, its `length` and every field of every child
inside N (u S + D) — N counted in the source and written down before the first run on a device, S and D from the oracle alone.
Nothing here is fitted to what the kernels give.  Each form also runs with a single ray."""
import numpy as np
import pytest

import fp32_interactions as fi
from optable_amd import abi

pytestmark = pytest.mark.gpu
ALL_FIELDS = abi.SEG_FIELDS + ("ray", "surface")


def _engine(scene):
    from optable_amd.engine import get_engine

    eng = get_engine()
    eng.upload(scene)
    return eng


def _launches(name, rays):
    """{launch: records in the reference's order} of the form's scene on `rays`, on every launch that takes it"""
    scene, K = fi.compiled(name), fi.max_trace_num(name)
    batch = fi.device_batch(rays)
    out = {}
    if name not in fi.BRANCHING:  # no hit of the fan branches: the default call, and the rolling lists where the library accepts the scene
        out["default"] = fi.table(name).trace_batch(batch, max_segments=2, scene=scene).to_host(reference_order=True)
        eng = _engine(scene)
        eng.set_option(abi.OPT_KERNEL, 2)
        try:
            segs = eng.trace(batch, 2)
            accepted = eng.last_launch()["kernel"] == 2
        except RuntimeError:
            accepted = False
        finally:
            eng.set_option(abi.OPT_KERNEL, 0)
        if accepted:
            out["rolling"] = segs.to_host(reference_order=True)
    out["tree"] = _engine(scene).trace_tree(batch, K).to_host(reference_order=True)
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _agree_bit_for_bit(name, out):
    first = next(iter(out))
    for launch, got in out.items():
        for f in ALL_FIELDS:
            assert got[f].dtype == out[first][f].dtype and np.array_equal(_bits(got[f]), _bits(out[first][f])), (name, launch, "differs from", first, "in", f)


def _report(name, n, launch, worst, bnd):
    # (the figures of DESIGN.md section 5: printed before anything is asserted)
    print(f"FP32I {name} n={n} {launch} excluded={int(bnd.excluded.sum())} " + " ".join(f"{f}={worst.get(f, float('nan')):.3f}" for f in abi.SEG_FIELDS))


@pytest.mark.parametrize("name", fi.NAMES)
def test_every_field_of_one_interaction_is_inside_its_bound(name, oracle):
    scene, rays, K, bnd = fi.reference(name)
    out = _launches(name, rays)
    assert "tree" in out and ("default" in out) == (name not in fi.BRANCHING), sorted(out)
    problems = []
    for launch, got in out.items():
        assert got["ox"].dtype == np.float32, (launch, got["ox"].dtype)
        bad, worst = fi.compare(bnd, rays, got)
        _report(name, len(rays["ox"]), launch, worst, bnd)
        problems += [f"{launch}: {b}" for b in bad]
    _agree_bit_for_bit(name, out)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("name", fi.NAMES)
def test_one_ray_alone(name, oracle):
    """n = 1: the first ray of the fan that is not excluded, as a batch of its own"""
    scene, rays, K, bnd = fi.reference(name)
    i = int(np.flatnonzero(~bnd.excluded)[0])
    out = _launches(name, fi.subset(rays, [i]))
    problems = []
    for launch, got in out.items():
        bad, worst = fi.compare(bnd, rays, got, only_rays={0: i})
        _report(name, 1, launch, worst, bnd)
        problems += [f"{launch}: {b}" for b in bad]
    _agree_bit_for_bit(name, out)
    assert not problems, "\n".join(problems)
