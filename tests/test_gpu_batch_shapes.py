"""Batched scans (tsd_batch_*) at their shape edges against the oracle: scanners of different beam counts and resolutions in one batch
(the registrations of all entries in the widest scanner's workgroup shape, helper grids sized by the largest count, ray-cast and
table launches as wide as the widest scan, k_mp_update's rotation table of robot 0 against a robot's own, the scan-window pool),
5 / 16 / 17 robots (helpers off; the one-pass push and the by-value ray cast at their limit; copied ray-cast entries and serial gated
pushes behind it), rounds in which robot 0 or everybody is gated out of the push.  The scenarios are tests/batch_shapes_ref.py's;
tests/test_cpu_batch_shapes.py shows with the oracle alone that each reaches its branch.  The oracle's side and the bars are those of
tests/test_gpu_batch.py::test_batch_matches_oracle: ray-cast hits, gates, pairs, iterations, state exact, poses through _compare, the
final grid cell for cell at 1e-5."""
import functools

import numpy as np
import pytest

from tests import batch_shapes_ref as B
from tests import helpers as H
import tests.test_gpu_batch as T

pytestmark = pytest.mark.gpu

AGAINST_ORACLE = ["mixed_two_360_first", "mixed_two_1081_first", "mixed_three_fov", "mixed_five", "robot0_gated_one_scanner",
                  "robot0_gated_mixed", "n16", "n17"]
MULTI_AGAINST_SERIAL = ["mixed_three_fov", "mixed_five", "robot0_gated_one_scanner", "robot0_gated_mixed", "n16"]


@functools.lru_cache(maxsize=None)
def _device_run(name, multi):
    """one device run of a scenario beside the oracle (compared per round and robot inside), shared by the tests that need it"""
    from oracle import pyoracle
    pyoracle.build()
    scn = B.SCENARIOS[name]
    seeded = []

    def compare(k, i, ro, sr):
        seeded.append((int(sr.icp.reserved), int(sr.icp.n_scene)))
        return T._compare(k, i, ro, sr)

    run = B.drive(pyoracle, scn, device=True, multi=multi, compare=compare)
    run["seeded"] = seeded
    print(f"{name} ({'one-pass' if multi else 'serial'} pushes): worst pose difference {run['worst']:.3e} m, {run['worst_rad']:.3e} rad; "
          f"scene points seeded by helpers / scene points, per scan: {seeded}")
    return scn, run


@pytest.mark.parametrize("name", AGAINST_ORACLE)
def test_batch_shape_matches_oracle(oracle, name):
    scn, run = _device_run(name, True)
    H.assert_grids_equal(run["oracle_grid"], run["tiles"], 1e-5)
    assert len(run["device"]) == scn.rounds
    # step 0's helper workgroups run for batches of up to four scans and for none above (tsd_batch_begin): the count of scene points
    # that started from a helper's granules says which
    for s, n_scene in run["seeded"]:
        assert (0 <= s <= n_scene) if scn.n <= 4 else s == 0, (scn.n, run["seeded"])
    if scn.n <= 4:
        # every entry's helpers deliver, the narrow entries' too (their count is smaller than the grid's: 2 against 5 workgroup rows
        # beside a 1081-beam scan) -- in at least one round each: a registration that has waited 25 us for them searches itself
        for i in range(scn.n):
            assert any(s > 0 for s, _ in run["seeded"][i::scn.n]), (i, run["seeded"])
    if name.startswith("robot0_gated"):
        pushed = [[r[1] for r in rnd] for rnd in run["device"]]
        assert pushed == [[1, 1, 1], [0, 1, 1], [0, 1, 1], [0, 0, 0], [1, 1, 1]]


@pytest.mark.parametrize("name", MULTI_AGAINST_SERIAL)
def test_batch_shape_one_pass_equals_serial_pushes(oracle, name):
    """the assertion of test_gpu_batch.py::test_batch_push_in_one_pass_equals_serial_pushes across mixed scanners, gated rounds and
    16 robots: two device grids driven identically, tsd_debug_set_push_multi on and off -- every scan result, the accumulated push
    statistics, the grid's digest and every array of the canonical dump are bit-identical (and both equal the oracle's within the bar)"""
    scn, a = _device_run(name, True)
    _, b = _device_run(name, False)
    H.assert_grids_equal(b["oracle_grid"], b["tiles"], 1e-5)
    assert a["device"] == b["device"], "scan results differ between the one-pass and the serial pushes"
    assert a["stats"] == b["stats"], f"push statistics differ: {a['stats']} / {b['stats']}"
    assert a["stats"][1] >= sum(sum(m) for m in scn.moves) // 2
    assert a["digest"] == b["digest"], f"grid digests differ: {a['digest']} / {b['digest']}"
    for x, y in zip(a["tiles"], b["tiles"]):
        assert np.array_equal(x, y, equal_nan=True)


def test_mixed_batch_with_the_pre_registration_matches_oracle(oracle):
    """registration_mode 3 for a 360-beam and a 1081-beam robot in one batch, both armed every round (trials 40, control set 120 as in
    test_batch_with_the_pre_registration_matches_oracle): the batch orders its registrations behind the grid stream by event
    (`any_pre`), winner, candidate count, idx, i exact (asserted per round in the driver), everything else as above"""
    scn, run = _device_run("mixed_mode3", True)
    assert scn.armed and all("pre" in ro for ros in run["ros"] for ro in ros)
    H.assert_grids_equal(run["oracle_grid"], run["tiles"], 1e-5)
