"""tsd_align_points / tsd_map_align on the device against the numpy restatement of tests/align_ref.py (whose fairness
tests/test_cpu_align.py shows): coarse scores uint32 for uint32, one accumulation of the refinement within the summation bound, the
refined poses within 10 eps of the restatement's, the call's invariants, and the end-to-end path down to tsd_fuse and SlamFleet.align.

The scenes are align_ref.scene's (512^2 cells of 0.05 m, oracle-built, uploaded with upload_tiles).  dst = map B, src = map A.
"""
import ctypes as C
import math

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, facade, synth
from tests import align_ref as A
from tests import group_merge_ref as GR
from tests import reloc_ref as R

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY = -1, -5
U = 2.0 ** -53


def upload(sc, dump):
    g = capi.TsdGridDevice(sc.gc.map_size_log2, sc.gc.cell_size, sc.gc.max_trunc)
    g.upload_tiles(*dump)
    return g


def grids(name):
    """(B, A) of a scene on the device (the test's own: every grid is closed when its test ends)"""
    sc = A.scene(name)
    return upload(sc, sc.dump_b), upload(sc, sc.dump_a)


def align(g, sc, points=None, **kw):
    a = dict(sc.lattice, pivot=sc.pivot, K=A.K, iterations=A.ITERATIONS)
    a.update(kw)
    return g.align_points(sc.points if points is None else points, **a)


def lever_distance(sc, m, c, s, rec):
    """the lever metric between a device state and a restated one"""
    da = math.atan2(s, c) - math.atan2(rec["s"], rec["c"])
    return max(math.hypot(m[0] - rec["m"][0], m[1] - rec["m"][1]), sc.lever * abs(math.atan2(math.sin(da), math.cos(da))))


# ------------------------------------------------------------------------------------------------------------------ scores
def test_scores_equal_the_restatement():
    sc = A.scene("diff")
    g, _ = grids("diff")
    out = align(g, sc, K=1, iterations=0)
    got = g.debug_align_scores().reshape(A.NTHETA, A.NXY, A.NXY)
    want = A.scene_scores("diff")
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert out["stride"] == 1 and out["n"] == len(sc.points)
    # the table the host fills in for a NULL cos_sin is libm's: the same volume
    align(g, sc, K=1, iterations=0, cos_sin=None, theta0=sc.theta0, dtheta=A.DTHETA)
    assert np.array_equal(g.debug_align_scores().reshape(A.NTHETA, A.NXY, A.NXY), want)


SCORE_EDGES = ["nx1", "ntheta1", "n1", "n63", "n64", "n65", "n2048", "n2049", "n4097", "border", "share_rotations", "share_single_position"]


@pytest.mark.parametrize("case", SCORE_EDGES)
def test_scores_on_edge_shapes(case):
    sc = A.scene("diff")
    g, _ = grids("diff")
    pts, table, pivot = sc.points, sc.table[10:15], sc.pivot
    lat = dict(x0=sc.x0 + 9 * A.STEP, y0=sc.y0 + 9 * A.STEP, step_xy=A.STEP, nx=5, ny=5)
    stride = 1
    if case == "nx1":
        lat.update(nx=1, ny=6); table = sc.table[8:15]
    elif case == "ntheta1":
        table = sc.table[12:13]
    elif case == "border":
        # 30 x 30 nodes, 1 m apart, from 2 m outside the grid's corner to beyond its far border, the list and a copy of it stretched about
        # the pivot: points are carried over the border, into tiles no scan initialised, onto NaN cells and into the halo strip
        lat = dict(x0=-2.0, y0=-2.0, step_xy=1.0, nx=30, ny=30); table = sc.table[::9]
        pts = np.concatenate([sc.points, (sc.points - np.array(pivot)) * 1.7 + np.array(pivot)])[:2048]
    elif case == "share_rotations":
        lat.update(nx=5, ny=3); table = sc.table[:7]           # 15 positions, 7 rotations: workgroups of 4 and of 3 rotations
    elif case == "share_single_position":
        lat.update(nx=1, ny=1, x0=sc.x0 + 11 * A.STEP, y0=sc.y0 + 12 * A.STEP); table = sc.table[:13]     # 13 rotations over 4 workgroups
    else:
        n = int(case[1:])
        # (beyond the list's length: a synthetic list made by repeating points)
        pts = np.concatenate([sc.points] * 3)[:n] if n > len(sc.points) else sc.points[700:700 + n]
        stride = (n + 2047) // 2048
    want = A.scores(sc.view_b, pts, pivot, lat["x0"], lat["y0"], lat["step_xy"], lat["nx"], lat["ny"], table)
    assert want.any()
    if case == "border":
        rel, _ = A.coarse_points(pts, pivot)
        seen, halo = set(), 0
        for iy in range(0, 30, 3):
            for ix in range(0, 30, 3):
                for c, s in table:
                    wx = (c * rel[:, 0] - s * rel[:, 1]) + (lat["x0"] + ix * 1.0); wy = (s * rel[:, 0] + c * rel[:, 1]) + (lat["y0"] + iy * 1.0)
                    st, _ = sc.view_b.bilinear(wx, wy)
                    seen |= set(st.tolist())
                    ok = st == R.SUCCESS
                    halo += int(np.count_nonzero(ok & ((np.floor(wx / sc.cs - 0.5).astype(np.int64) & 31) == 31)))
                    halo += int(np.count_nonzero(ok & ((np.floor(wy / sc.cs - 0.5).astype(np.int64) & 31) == 31)))
        assert seen == {R.SUCCESS, R.INVALIDINDEX, R.EMPTYPARTITION, R.ISNAN} and halo > 0
    out = g.align_points(pts, pivot=pivot, cos_sin=table, ntheta=len(table), theta_wraps=False, K=4, iterations=0, **lat)
    assert out["stride"] == stride and out["n"] == len(pts)
    got = g.debug_align_scores().reshape(len(table), lat["ny"], lat["nx"])
    assert np.array_equal(got, want), f"{case}: {np.count_nonzero(got != want)} scores differ"
    idx, sco = R.peaks(want, want.shape, False, 4)
    recs = g.debug_align_peaks()
    assert [r["idx"] for r in recs] == idx.tolist() and [r["score"] for r in recs] == sco.tolist()


# --------------------------------------------------------------------------------------- the two searches' score volumes
def _both_searches():
    """one context that holds map A (the "self" scene: the alignment's dst and, the same 12 scans, the relocalisation's map) with a
    relocalisation and an alignment over small lattices on it: (grid, reloc(lattice, table) -> restated volume,
    align(lattice, table) -> restated volume)"""
    sa, sr = A.scene("self"), R.scene(360)
    g = upload(sa, sa.dump_b)
    icp = g.icp_params(R.ICP["iterations"], R.ICP["dist_max"], R.ICP["dist_min"])

    def reloc(lat, table, points=sr.points, restate=True):
        g.relocalize(points, sr.rays_local, sr.data, sr.mask, R.MIN_RANGE, R.MAX_RANGE, icp, cos_sin=table, ntheta=len(table), K=1, **lat)
        if restate:
            want, gate = R.scores(sa.view_b, points, lat["x0"], lat["y0"], lat["step_xy"], lat["nx"], lat["ny"], table)
            assert gate.any() and want.any()
            return want.reshape(-1)

    def align(lat, table, points=sa.points, restate=True):
        g.align_points(points, pivot=sa.pivot, cos_sin=table, ntheta=len(table), K=1, iterations=0, **lat)
        if restate:
            want = A.scores(sa.view_b, points, sa.pivot, lat["x0"], lat["y0"], lat["step_xy"], lat["nx"], lat["ny"], table)
            assert want.any()
            return want.reshape(-1)
    return g, sa, sr, reloc, align


def test_the_two_score_volumes_are_independent():
    """a relocalisation leaves the alignment's volume as it was and the other way round; each search's own is the restatement's"""
    g, sa, sr, reloc, align = _both_searches()
    want_r = reloc(dict(x0=sr.x0 + 10 * R.STEP, y0=sr.y0 + 10 * R.STEP, step_xy=R.STEP, nx=3, ny=3), sr.table[10:14])
    assert np.array_equal(g.debug_reloc_scores(), want_r) and g.debug_align_scores().size == 0
    want_a = align(dict(x0=sa.x0 + 9 * A.STEP, y0=sa.y0 + 10 * A.STEP, step_xy=A.STEP, nx=4, ny=2), sa.table[11:14])
    assert np.array_equal(g.debug_align_scores(), want_a) and np.array_equal(g.debug_reloc_scores(), want_r)
    want_r = reloc(dict(x0=sr.x0 + 9 * R.STEP, y0=sr.y0 + 11 * R.STEP, step_xy=R.STEP, nx=2, ny=3), sr.table[9:14])
    assert np.array_equal(g.debug_reloc_scores(), want_r) and np.array_equal(g.debug_align_scores(), want_a)
    assert want_r.size == 30 and want_a.size == 24
    g.close()


@pytest.mark.parametrize("search", ["reloc", "align"])
def test_a_volume_beyond_2_23_candidates_is_given_back_and_a_small_one_kept(search):
    """512 x 512 x 33 candidates (just over 2^23) over the whole grid: nothing of it stays with the context; the small search that
    follows is kept, and the other search's volume is not touched by either"""
    g, sa, sr, reloc, align = _both_searches()
    small_r = dict(x0=sr.x0 + 10 * R.STEP, y0=sr.y0 + 10 * R.STEP, step_xy=R.STEP, nx=3, ny=3)
    small_a = dict(x0=sa.x0 + 9 * A.STEP, y0=sa.y0 + 10 * A.STEP, step_xy=A.STEP, nx=4, ny=2)
    want_r, want_a = reloc(small_r, sr.table[10:14]), align(small_a, sa.table[11:14])
    big = dict(x0=0.5 * sa.cs, y0=0.5 * sa.cs, step_xy=sa.cs, nx=512, ny=512)
    assert 512 * 512 * 33 > 1 << 23
    if search == "reloc":
        reloc(big, sr.table[:33], restate=False)
        assert g.debug_reloc_scores().size == 0 and np.array_equal(g.debug_align_scores(), want_a)
        assert np.array_equal(reloc(small_r, sr.table[10:14]), g.debug_reloc_scores())
    else:
        align(big, sa.table[:33], points=sa.points[::len(sa.points) // 64][:64], restate=False)
        assert g.debug_align_scores().size == 0 and np.array_equal(g.debug_reloc_scores(), want_r)
        assert np.array_equal(align(small_a, sa.table[11:14]), g.debug_align_scores())
    g.close()


# -------------------------------------------------------------------------------------------------------------------- sums
def _sums_poses(sc):
    idx, _, recs = A.scene_records("diff")
    m, c, s = A.start_of(sc, idx[0])
    th = sc.truth[2] + math.radians(40.0)
    return {"peak": (m, c, s), "end": (recs[0]["m"], recs[0]["c"], recs[0]["s"]),
            "far": ((sc.truth[0] + 1.0, sc.truth[1] + 0.7), math.cos(th), math.sin(th))}


@pytest.mark.parametrize("pose", ["peak", "end", "far"])
def test_sums_equal_the_restatement(pose):
    """n_ok exact; every sum within (n + 64) * 2^-53 * sum |term| of numpy's: n - 1 additions in whatever order plus the roundings of one
    term (its dozen operations, a square root and two divisions).  Observed on an MI355X: at most 0.021 of the bound (at the end pose; 0.0013 at the other two)."""
    sc = A.scene("diff")
    g, _ = grids("diff")
    m, c, s = _sums_poses(sc)[pose]
    worst = 0.0
    for n in (1, 2, 3, 1023, 1024, 1025, len(sc.points)):
        pts = sc.points[:n] if n > 3 else sc.points[900:900 + n]
        want, n_ok, mag = A.accumulate(sc.view_b, pts - np.array(sc.pivot), m, c, s, A.V_CUT, sc.max_trunc)
        got, got_ok = g.debug_align_sums(pts, sc.pivot, m, c, s, A.V_CUT)
        assert got_ok == n_ok, f"{pose}, n = {n}: n_ok {got_ok}, the restatement's {n_ok}"
        bound = (n + 64) * U * mag
        err = np.abs(got - want)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
        assert np.all(err <= bound), f"{pose}, n = {n}: {err} against {bound}"
    full = A.accumulate(sc.view_b, sc.points - np.array(sc.pivot), m, c, s, A.V_CUT, sc.max_trunc)
    print(f"sums at '{pose}': worst error / bound = {worst:.3g}; n_ok = {full[1]}, sum w = {full[0][9]:.1f}")
    # the poses are what their names say: few points inside the cut half a step and three degrees off, most of them at the end, a
    # handful in the wrong basin
    assert {"peak": 100 < full[0][9] < 900, "end": full[0][9] > 1000, "far": full[0][9] < 100}[pose] and full[1] >= 3


# -------------------------------------------------------------------------------------------------------------- refinement
@pytest.mark.parametrize("name", ["self", "same", "diff"])
def test_refined_peaks_equal_the_restatement(name):
    """For every peak whose restatement converges the device's final state lies within 10 eps of the restatement's in the lever
    metric: both stop below eps at a contraction of at most 1/2, and a discrete decision (the gain rule, the stopping iteration) may
    fall differently by rounding.  Observed on an MI355X: 5.7e-15 (self), 3.6e-15 (same), 2.8e-15 (diff) over the 11 / 11 / 12
    converged peaks -- no discrete decision fell differently on these scenes."""
    sc = A.scene(name)
    g, _ = grids(name)
    idx, sco, recs = A.scene_records(name)
    out = align(g, sc)
    dev = g.debug_align_peaks()
    assert out["n_peaks"] == out["n_refined"] == len(dev) == len(idx)
    assert [r["idx"] for r in dev] == idx.tolist() and [r["score"] for r in dev] == sco.tolist()
    worst, compared = 0.0, 0
    for d, r in zip(dev, recs):
        if r["status"] != A.CONVERGED:
            continue
        compared += 1
        dist = lever_distance(sc, d["m"], d["c"], d["s"], r)
        worst = max(worst, dist)
        assert d["status"] == capi.ALIGN_CONVERGED, f"peak {d['idx']}: status {d['status']} after {d['iterations']} steps"
        assert dist <= 10.0 * A.EPS, f"peak {d['idx']}: {dist} from the restatement"
        assert abs(math.hypot(d["c"], d["s"]) - 1.0) <= 4 * U
    print(f"{name}: {compared} converged peaks compared, worst lever distance {worst:.3g}")
    assert compared >= 8
    # the result is the winner's
    w = max((j for j in range(len(dev)) if dev[j]["status"] != capi.ALIGN_DEGENERATE), key=lambda j: (dev[j]["sums"][9], -j))
    assert out["idx"] == dev[w]["idx"] and out["weight_sum"] == dev[w]["sums"][9] and out["found"]
    assert np.array_equal(out["T"], A.transform(dict(c=dev[w]["c"], s=dev[w]["s"], m=dev[w]["m"]), sc.pivot))
    assert np.array_equal(out["info"], dev[w]["sums"][:6]) and out["n_ok"] == dev[w]["n_ok"]
    d, a = A.map_error(out["T"], sc.D, sc.side)
    assert (d <= 1e-5 and a <= 1e-6 and out["rms"] <= 1e-5) if name == "self" else (d <= 0.5 * sc.cs and a <= 1e-3)


def test_zero_and_one_iteration():
    sc = A.scene("diff")
    g, _ = grids("diff")
    idx, _, _ = A.scene_records("diff")
    out = align(g, sc, iterations=0)
    dev = g.debug_align_peaks()
    for d, i in zip(dev, idx):
        m, c, s = A.start_of(sc, i)
        assert (d["m"], d["c"], d["s"], d["iterations"], d["status"], d["gain"]) == (m, c, s, 0, capi.ALIGN_MAXITER, 1.0)
    assert not out["found"] and not out["converged"] and out["iterations"] == 0
    w = [d["idx"] for d in dev].index(out["idx"])
    m, c, s = A.start_of(sc, out["idx"])
    assert out["coarse"] == (m[0], m[1], c, s)
    assert np.array_equal(out["T"], A.transform(dict(c=c, s=s, m=m), sc.pivot)) and out["score"] == dev[w]["score"]
    # one step: the sums agree to ~1e-13 relative, the 3 x 3 solve amplifies that by the condition of A in the lever's units (< 1e4),
    # the step is below 1 m: 1e-8 leaves two orders of magnitude
    align(g, sc, iterations=1)
    for d, i in zip(g.debug_align_peaks(), idx):
        m, c, s = A.start_of(sc, i)
        r = A.refine(sc.view_b, sc.points, sc.pivot, m, c, s, 1, sc.max_trunc, sc.lever)
        if r["status"] == A.DEGENERATE:
            assert d["status"] == capi.ALIGN_DEGENERATE
            continue
        assert d["iterations"] == 1 and d["status"] == r["status"]
        assert lever_distance(sc, d["m"], d["c"], d["s"], r) <= 1e-8


def test_peak_counts():
    sc = A.scene("diff")
    g, _ = grids("diff")
    align(g, sc)
    base = g.debug_align_peaks()
    align(g, sc, K=1)
    one = g.debug_align_peaks()
    assert len(one) == 1 and one[0]["raw"] == base[0]["raw"]
    out = align(g, sc, K=64)
    many = g.debug_align_peaks()
    idx, sco = R.peaks(A.scene_scores("diff"), (A.NTHETA, A.NXY, A.NXY), True, 64)
    assert len(many) == len(idx) == out["n_peaks"] and len(many) > A.K
    assert [r["idx"] for r in many] == idx.tolist()
    assert [r["raw"] for r in many[:A.K]] == [r["raw"] for r in base]
    # fewer peaks than K: a lattice of one node has one peak at most
    m, c, s = A.start_of(sc, base[0]["idx"])
    out = g.align_points(sc.points, x0=m[0], y0=m[1], step_xy=A.STEP, nx=1, ny=1, ntheta=1, cos_sin=[c, s], pivot=sc.pivot, K=16,
                         iterations=A.ITERATIONS)
    assert out["n_peaks"] == 1 and len(g.debug_align_peaks()) == 1 and out["found"]
    assert g.debug_align_peaks()[0]["raw"][8:] == base[0]["raw"][8:]            # (the candidate index and score aside)


def test_degenerate_lists_are_no_error():
    sc = A.scene("diff")
    g, _ = grids("diff")
    out = align(g, sc, points=sc.points[:2])
    assert not out["found"] and out["idx"] == -1 and np.isnan(out["T"]).all() and out["n"] == 2
    assert out["n_peaks"] >= 1 and all(r["status"] == capi.ALIGN_DEGENERATE and r["n_ok"] <= 2 for r in g.debug_align_peaks())
    # every point in unseen space: no candidate scores, no peak
    corner = np.full((50, 2), 0.3) + np.linspace(0.0, 0.2, 50)[:, None]
    assert not A.scores(sc.view_b, corner, (0.3, 0.3), 0.3, 0.3, 0.05, 4, 4, R.rotation_table(4, 0.0, 0.1)).any()
    out = g.align_points(corner, x0=0.3, y0=0.3, step_xy=0.05, nx=4, ny=4, ntheta=4, theta0=0.0, dtheta=0.1, pivot=(0.3, 0.3), K=8,
                         iterations=10)
    assert not out["found"] and out["n_peaks"] == 0 and g.debug_align_peaks() == [] and not g.debug_align_scores().any()
    assert align(g, sc)["found"]


# -------------------------------------------------------------------------------------- invariants and the end-to-end path
def test_same_call_twice_same_bits_and_the_grids_stay():
    sc = A.scene("diff")
    gb, ga = grids("diff")
    db, da, tb, ta = gb.digest(), ga.digest(), gb.download_tile_state(), ga.download_tile_state()
    first = align(gb, sc)
    rec1 = [r["raw"] for r in gb.debug_align_peaks()]
    second = align(gb, sc)
    assert first["raw"] == second["raw"] and rec1 == [r["raw"] for r in gb.debug_align_peaks()]
    m1 = gb.align_to(ga, **sc.lattice, K=A.K, iterations=A.ITERATIONS)
    m2 = gb.align_to(ga, **sc.lattice, K=A.K, iterations=A.ITERATIONS)
    assert m1["raw"] == m2["raw"] and m1["found"]
    assert gb.digest() == db and ga.digest() == da
    for before, after in ((tb, gb.download_tile_state()), (ta, ga.download_tile_state())):
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # the device list: src's surface list, staged by the caller, gives what the host list gives
    n = ga.surface_extract()
    xy, _, _ = ga.surface_fetch(0, n, normals=False)
    assert np.array_equal(xy, sc.points_raw)
    host = align(gb, sc, points=xy)
    dev = gb.align_points(None, **dict(sc.lattice, pivot=sc.pivot, K=A.K, iterations=A.ITERATIONS), device_ptr=ga.surface_dev()[0], n=n)
    assert host["raw"] == dev["raw"]


def test_refusals_allocate_nothing_and_a_good_call_follows():
    sc = A.scene("diff")
    g = upload(sc, sc.dump_b)                       # a context of its own: nothing has been allocated for it yet
    ref, other = grids("diff")
    d0 = g.digest()

    def refused(code, text, **kw):
        with pytest.raises(capi.TsdError):
            align(g, sc, **kw)
        assert g.last_rc == code, (kw, g.last_rc)
        assert g.lib.tsd_last_error(g.h).decode() == "tsd_align_points: " + text, kw

    K_RANGE, STEPS, SHAPE = "K outside 1 .. TSD_RELOC_MAX_PEAKS", "iterations outside 0 .. 64", "nx, ny, ntheta must be >= 1"
    ORIGIN, TABLE = "x0, y0 finite and step_xy > 0", "cos_sin is not finite"
    POINT = "a point is not finite or further than TSD_RELOC_MAX_REACH grid widths away"
    refused(E_ARG, K_RANGE, K=0); refused(E_ARG, K_RANGE, K=65)
    refused(E_ARG, STEPS, iterations=-1); refused(E_ARG, STEPS, iterations=65)
    refused(E_ARG, SHAPE, nx=0); refused(E_ARG, ORIGIN, step_xy=0.0); refused(E_ARG, ORIGIN, x0=float("nan"))
    refused(E_CAPACITY, "nx * ny * ntheta > TSD_RELOC_MAX_CANDIDATES", nx=1 << 14, ny=1 << 14, step_xy=1e-4)
    refused(E_ARG, "the lattice reaches further than TSD_RELOC_MAX_REACH grid widths from the grid", x0=-4.0 * sc.side - 1.0)
    refused(E_ARG, "v_cut outside (0, 1]", v_cut=1.5); refused(E_ARG, "v_cut outside (0, 1]", v_cut=-0.1)
    refused(E_ARG, "eps must be > 0", eps=-1.0); refused(E_ARG, "lever is not finite", lever=float("inf"))
    refused(E_ARG, "the pivot is not finite or further than TSD_RELOC_MAX_REACH grid widths away", pivot=(float("inf"), 0.0))
    refused(E_ARG, "min_overlap / max_rms is NaN", min_overlap=float("nan"))
    refused(E_ARG, "without a cos_sin table, theta0 and a non-zero dtheta are needed", cos_sin=None, dtheta=0.0)
    bad = sc.table.copy(); bad[7, 0] = np.nan
    refused(E_ARG, TABLE, cos_sin=bad)
    far = sc.points.copy(); far[3, 1] = 5.0 * sc.side
    refused(E_ARG, POINT, points=far)
    nan = sc.points.copy(); nan[0, 0] = np.nan
    refused(E_ARG, POINT, points=nan)
    refused(E_ARG, "no point", points=np.zeros((0, 2)))
    # several bad arguments: the one that is checked first is named -- K, iterations, the lattice (shape, then x0 / y0 / step_xy), the
    # table, the pivot
    refused(E_ARG, K_RANGE, K=0, nx=0)
    refused(E_ARG, SHAPE, nx=0, x0=float("nan"))
    refused(E_ARG, TABLE, cos_sin=bad, pivot=(float("inf"), 0.0))
    assert g.lib.tsd_align_points(g.h, None, None, 0, 0, None) == E_ARG
    assert g.debug_align_scores().size == 0 and g.debug_align_peaks() == []       # nothing was searched, nothing is kept
    # dst == src, src missing
    with pytest.raises(capi.TsdError):
        g.align_to(g, **sc.lattice)
    assert g.last_rc == E_ARG
    with pytest.raises(capi.TsdError):
        g.align_to(None, **sc.lattice)
    # while a scan of either context is in flight
    from oracle import pyoracle as O
    rays_local = O.rays_local(sc.geo.beams, sc.geo.angle_min, sc.geo.angle_increment)
    s = capi.TsdSensorDevice(g, sc.geo.beams, sc.geo.angle_increment, sc.geo.angle_min, R.MAX_RANGE, R.MIN_RANGE, R.LOW_REFL)
    pose = sc.D @ synth.pose_matrix(*sc.poses[-1])
    s.set_pose(pose, R.rays_world(pose, rays_local, sc.gc.cell_size), rays_local)
    data, mask = O.ingest_f32(sc.world.scan(*sc.poses[-1], sc.geo), R.MAX_RANGE, sc.geo.angle_increment)
    gates = capi.GateParams(1.0, 0.5, 10.0, 10.0)      # (a push gate nothing passes: the scan leaves the grid as it is)
    prm = g.icp_params(R.ICP["iterations"], R.ICP["dist_max"], R.ICP["dist_min"])
    rg, mk = np.ascontiguousarray(data), np.ascontiguousarray(mask, dtype=np.uint8)
    g._check(g.lib.tsd_scan_submit(s.h, capi._d(rg), capi._u8(mk), None, C.byref(prm), C.byref(gates)), "tsd_scan_submit")
    refused(E_ARG, "a scan of this context is in flight (collect it first)")
    with pytest.raises(capi.TsdError):
        g.align_to(other, **sc.lattice)
    assert g.last_rc == E_ARG
    with pytest.raises(capi.TsdError):
        other.align_to(g, **sc.lattice)               # ... as the source as well
    assert other.last_rc == E_ARG
    with pytest.raises(capi.TsdError):
        g.debug_align_sums(sc.points, sc.pivot, (1.0, 1.0), 1.0, 0.0)
    res = capi.ScanResult()
    g._check(g.lib.tsd_scan_collect(s.h, C.byref(res)), "tsd_scan_collect")
    assert not res.pushed and g.digest() == d0
    s.close()
    # the good call that follows
    out = align(g, sc)
    assert out["found"] and out["raw"] == align(ref, sc)["raw"]
    g.close()


@pytest.mark.parametrize("name", ["self", "diff", "cells"])
def test_map_align_end_to_end(name):
    """tsd_map_align(B, A): A's surface list is extracted and staged with the half-cell offset on the device; the bounds are the CPU
    tests' (tests/test_cpu_align.py)"""
    sc = A.scene(name)
    gb, ga = grids(name)
    gb.profile(True)
    out = gb.align_to(ga, **sc.lattice, K=A.K, iterations=A.ITERATIONS)
    gb.profile(False)
    d, a = A.map_error(out["T"], sc.D, sc.side)
    print(f"{name}: {d:.3g} m, {a:.3g} rad, rms {out['rms']:.3g}, overlap {out['overlap']:.3f}, {out['iterations']} steps, "
          f"search {out['search_ms']:.3f} ms, refinement {out['refine_ms']:.3f} ms")
    assert out["found"] and out["converged"] and out["n"] == len(sc.points) and out["search_ms"] > 0.0 and out["refine_ms"] > 0.0
    # the same as the list staged on the host: the default pivot is the centre of src's grid, the offset cs_src / 2
    assert out["raw"][:-16] == align(gb, sc)["raw"][:-16]
    if name == "self":
        assert d <= 1e-5 and a <= 1e-6 and out["rms"] <= 1e-5
        assert out["cell_off"] == (0, 0) and out["cell_error"] < 1e-3
    else:
        assert d <= 0.5 * sc.cs and a <= 1e-3
    off, err = A.cell_shift(out["T"], sc.cs, sc.cells)
    assert out["cell_off"] == off and abs(out["cell_error"] - err) <= 1e-9
    # found = converged and overlap >= min_overlap and rms <= max_rms
    assert not gb.align_to(ga, **sc.lattice, K=A.K, iterations=A.ITERATIONS, min_overlap=0.99)["found"]
    assert not gb.align_to(ga, **sc.lattice, K=A.K, iterations=A.ITERATIONS, max_rms=1e-9)["found"]
    if name == "cells":
        assert out["cell_off"] == A.CELLS_SHIFT and out["cell_error"] < 0.5
        # the shift goes into tsd_fuse as it is: the fusion with it is the fusion with the offsets the maps were built with
        fused = capi.TsdGridDevice(sc.gc.map_size_log2, sc.gc.cell_size, sc.gc.max_trunc)
        fused.fuse_from([gb, ga], [(0, 0), out["cell_off"]])
        d_aligned = fused.digest()
        fused.fuse_from([gb, ga], [(0, 0), A.CELLS_SHIFT])
        assert fused.digest() == d_aligned and d_aligned["cells_valid"] > gb.digest()["cells_valid"]
        fused.close()
    if name == "diff":
        assert out["cell_error"] > 0.5                 # a rotated transform is not a whole-cell shift


def test_an_empty_source_map_is_no_error():
    sc = A.scene("diff")
    gb, _ = grids("diff")
    empty = capi.TsdGridDevice(sc.gc.map_size_log2, sc.gc.cell_size, sc.gc.max_trunc)
    out = gb.align_to(empty, **sc.lattice)
    assert not out["found"] and out["n"] == 0 and out["n_peaks"] == 0 and out["idx"] == -1 and gb.debug_align_peaks() == []
    empty.close()


def test_slam_fleet_align():
    """two nodes that mapped the same room, their grids placed 0.6 m / -0.425 m apart: the pose of node 1's map in node 0's is the
    offset between the robots' start poses in their grids, within half a cell"""
    gc = synth.GridConfig(10, 0.025)
    geo = synth.ScanGeometry.full_circle_360()
    world = synth.World("room", gc)
    scans = synth.scans_for(world, geo, synth.trajectory(world, 6))
    offsets = [(0.0, 0.0), (0.6, -0.425)]
    nodes = [facade.SlamNode(facade.node_params(gc, geo, x_offset=xo, y_offset=yo, occ_grid_time_interval=1000.0), synchronous=True,
                             name=f"tsd_slam_{i}") for i, (xo, yo) in enumerate(offsets)]
    fleet = facade.SlamFleet(nodes)
    try:
        for k in range(len(scans)):
            for n in nodes:
                n.laser(scans[k], geo.angle_min, geo.angle_increment)
        cs, side = gc.cell_size, gc.cells * gc.cell_size
        # node 1's cell (x, y) is node 0's cell (x + ox, y + oy): the fleet's own placement of the grids (tsd_fuse's convention)
        want = tuple(GR.cell_offset(GR.map_origin(gc.cells, cs, offsets[1][a]), GR.map_origin(gc.cells, cs, offsets[0][a]), cs) for a in (0, 1))
        assert want == (-24, 17)
        land = (0.5 * side + want[0] * cs, 0.5 * side + want[1] * cs)          # where the centre of node 1's grid lies in node 0's
        digests = [n.grid().digest() for n in nodes]
        # the lattice: 12 x 12 x 9 at 0.05 m and half a degree, the truth 5.4 / 5.7 / 4.3 steps from its corner.  It is this fine because
        # a node must lie inside the cut: v_cut * max_trunc = 0.056 m here, for walls that stand 6 .. 10 m from the pivot
        lat = dict(step_xy=0.05, nx=12, ny=12, ntheta=9, theta0=-4.3 * math.radians(0.5), dtheta=math.radians(0.5), K=8, iterations=64)
        out = fleet.align(0, 1, x0=land[0] - 5.4 * 0.05, y0=land[1] - 5.7 * 0.05, **lat)
        print(f"fleet: translation ({out['T'][0, 2]:.5f}, {out['T'][1, 2]:.5f}), cell_off {out['cell_off']}, cell_error {out['cell_error']:.3g}, "
              f"n = {out['n']}, stride {out['stride']}")
        assert out["found"] and out["n"] > 1000
        assert math.hypot(out["T"][0, 2] - want[0] * cs, out["T"][1, 2] - want[1] * cs) <= 0.5 * cs
        assert abs(math.atan2(out["T"][1, 0], out["T"][0, 0])) <= 1e-3
        assert out["cell_off"] == want and out["cell_error"] < 0.5
        assert [n.grid().digest() for n in nodes] == digests
        with pytest.raises(capi.TsdError):
            fleet.align(1, 1, x0=0.0, y0=0.0, step_xy=0.1, nx=1, ny=1, ntheta=1, cos_sin=[1.0, 0.0])
        back = fleet.align(1, 0, x0=0.5 * side - want[0] * cs - 5.4 * 0.05, y0=0.5 * side - want[1] * cs - 5.7 * 0.05, **lat)
        assert back["found"] and back["cell_off"] == (-want[0], -want[1])
    finally:
        fleet.close()
        for n in nodes:
            n.close()
