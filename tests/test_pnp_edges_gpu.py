"""The device PnP (centerpose_amd/csrc/pnp.hip) at its branch switches, singular poses, validity patterns, cameras and
placements, useless inputs and launch shapes, on the cases of tests/pnp_edge_cases.py (whose premises
tests/test_pnp_edges_cpu.py checks on the oracle alone).

* per family, against the float64 oracle: status, pose (geodesic angle, tvec), the eight projected points, the reprojection
  error, the OpenGL location, both quaternions element for element (NaN elements included), the Levenberg-Marquardt
  iteration count (which tells the DLT start from the homography start) and the valid-point count; on exact data also
  against the generating pose.  Limits: pnp_edge_cases.LIMITS / GENERATING_LIMITS, set from the oracle alone.
* a row is a function of its own inputs: bit-identical alone, in a small batch, padded to 256 and 257, at every offset
  modulo 4 of the four-detections-per-wavefront shape, next to every kind of neighbour, in reversed order.
* the rare list with every row rare at N = 300; cp_pnp_from_post above 256 slots; useless inputs.
Each test is one or a few cp_pnp_solve calls on at most a few hundred rows (whole module: 3 s on an MI355X).
"""
import numpy as np
import pytest
import torch

from centerpose_amd import hip
from oracle import pnp as opnp
from tests import pnp_edge_cases as pc

pytestmark = pytest.mark.gpu


def _solve(device, c):
    out = hip.pnp_solve(torch.from_numpy(c.pts).to(device), torch.from_numpy(c.scale).to(device),
                        torch.from_numpy(c.cam).to(device)).cpu().numpy()
    assert out.shape == (len(c.names), hip.PNP_STRIDE)
    return out


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _self_consistent(row, pts, scale, cam):
    """A status-1 row against its OWN pose, recomputed with the oracle's projection: valid-point count, RMS reprojection
    error of the given points (which slot belongs to which vertex, which slots are valid), the eight projected vertices, the
    OpenGL location, and finite numbers everywhere but in quaternion elements that are 0 / 0 (rotation vector exactly zero)."""
    valid = ~((pts[:, 0] < -5000) | (pts[:, 1] < -5000))
    assert int(row[35]) == int(valid.sum())
    assert np.isfinite(row[1:24]).all() and np.isfinite(row[28:31]).all() and np.isfinite(row[35:]).all()
    verts = pc.rel_verts(scale)
    obj = np.repeat(verts, len(pts) // 8, axis=0)
    K = pc.Kmat(cam)
    uv = opnp.project_points(obj[valid], row[1:4], row[4:7], K)
    rms = float(np.linalg.norm(uv - pts[valid].astype(np.float64)) / np.sqrt(2 * valid.sum()))
    span = 1.0 + np.abs(uv).max()
    assert abs(rms - row[7]) <= 1e-9 * span, (rms, row[7])
    np.testing.assert_allclose(row[8:24].reshape(8, 2), opnp.project_points(verts, row[1:4], row[4:7], K), rtol=0, atol=1e-9 * span)
    np.testing.assert_array_equal(row[28:31], pc.M_GL @ row[4:7])
    assert np.isfinite(row[24:28]).all() or not row[1:4].any()
    Rg = pc.M_GL @ opnp.rodrigues_to_matrix(row[1:4])
    with np.errstate(all="ignore"):
        q = opnp.axis_angle_quat_xyzw(opnp.matrix_to_rodrigues(Rg))
    assert pc.quat_diff(row[31:35], q) < 1e-6  # (sqrt conditioning of the near-pi branch: 1e-8 measured on the oracle)


def _check_family(fam, c, out, limits, gen_limits):
    """Every row of ``out`` against the oracle; prints the worst figure of each compared quantity before asserting."""
    rows = pc.oracle_rows(c)
    assert len(rows) <= 200
    defined = getattr(c, "defined", np.ones(len(rows), bool))
    worst = {q: 0.0 for q in pc.QUANTITIES}
    worst_gen = {"rot_deg": 0.0, "t_rel": 0.0}
    failures = []
    n_pose = 0
    for i, r in enumerate(rows):
        st = out[i, 0]
        if st == 1:
            _self_consistent(out[i], c.pts[i], c.scale[i], c.cam[i])
        if not defined[i]:  # under-determined correspondences: the reference has no defined answer (pnp_edge_cases.py)
            if st not in (0, 1, 2):
                failures.append((c.names[i], "status", st))
            continue
        if r.kind == "none":
            want = {"behind_camera": (2,), "solver_failed": (0,), "few_points": (-1,)}[r.why]
            if st not in want:
                failures.append((c.names[i], "oracle: %s, device status" % r.why, st))
            continue
        assert r.kind == "pose", (c.names[i], r.kind)
        if st != 1:
            failures.append((c.names[i], "oracle has a pose, device status", st))
            continue
        n_pose += 1
        d = pc.pose_diff(pc.device_pose(out[i]), r)
        for q in pc.QUANTITIES:
            worst[q] = max(worst[q], d[q])
            if not d[q] <= limits[q]:
                failures.append((c.names[i], q, d[q]))
        if int(out[i, 36]) != r.iters:
            failures.append((c.names[i], "LM iterations device / oracle", int(out[i, 36]), r.iters))
        if c.exact[i] and np.isfinite(c.R[i]).all():
            g = {"rot_deg": pc.geodesic_deg(opnp.rodrigues_to_matrix(out[i, 1:4]), c.R[i]),
                 "t_rel": float(np.linalg.norm(out[i, 4:7] - c.t[i]) / np.linalg.norm(c.t[i]))}
            for q in g:
                worst_gen[q] = max(worst_gen[q], g[q])
                if not g[q] <= gen_limits[q]:
                    failures.append((c.names[i], "generating pose " + q, g[q]))
    print("\n%s: %d rows, %d poses compared; worst vs oracle %s; worst vs generating pose %s" % (
        fam, len(rows), n_pose, {q: "%.1e" % v for q, v in worst.items()}, {q: "%.1e" % v for q, v in worst_gen.items()}))
    assert not failures, failures
    return rows, n_pose


@pytest.mark.parametrize("fam", list(pc.FAMILIES))
def test_family_vs_float64_oracle(device, fam):
    c = pc.FAMILIES[fam]()
    out = _solve(device, c)
    rows, n_pose = _check_family(fam, c, out, pc.LIMITS[fam], pc.GENERATING_LIMITS[fam])
    # the floor tests/test_pnp_edges_cpu.py establishes on the oracle: every row but the documented ones has a pose
    floor = {"planar_switch": 61, "singular_rotation": 71, "validity_patterns": 32, "validity_patterns_8": 16,
             "camera_and_placement": 58}[fam]
    assert n_pose >= floor, (n_pose, floor)
    if fam == "singular_rotation":
        # the 0 / 0 of axis_angle_quat is reached (OpenGL-frame angle below 1e-5: rot_to_rvec returns the zero vector), and
        # the planar_init failure's fall-back r = t = 0 is walked to the same end as the oracle's (behind the camera)
        assert sum(bool(np.isnan(out[i, 31:34]).all() and out[i, 34] == 1.0) for i in range(len(rows))) == 13
        assert out[c.planar_init_fails, 0] == 2 and out[c.planar_init_fails, 35] == 8
    # the same batch beyond 256 rows (four detections per wavefront): bit-identical rows
    n = len(c.names)
    big = _solve(device, pc.take(c, np.arange(300) % n))
    assert _same_bits(big, out[np.arange(300) % n])


@pytest.mark.parametrize("npts", [16, 8])
def test_row_is_a_function_of_its_own_inputs(device, npts):
    c = pc.mixed_rows(npts)
    n = len(c.names)
    ref = np.concatenate([_solve(device, pc.take(c, [i])) for i in range(n)])  # alone: N = 1
    st = ref[:, 0]
    print("\nstatuses alone:", dict(zip(*np.unique(st, return_counts=True))))
    assert set(st) <= {-1.0, 0.0, 1.0, 2.0}
    name = {nm: i for i, nm in enumerate(c.names)}
    if npts == 16:  # every way a row can end, both rare branches with and without a pose
        assert set(st) == {-1.0, 0.0, 1.0, 2.0}
        assert st[name["planar 0"]] == 1 and st[name["five points 0"]] == 1 and st[name["four coplanar points"]] == 0
        assert st[name["planar_init fails: face x=-w/2 edge-on"]] == 2 and st[name["no valid point"]] == -1
        assert st[name["u mirrored about the principal point"]] == 2 and st[name["all points NaN"]] == 0
    assert _same_bits(_solve(device, c), ref)                                  # together, one workgroup each
    for N in (256, 257):                                                       # the last and the first size of each shape
        idx = np.arange(N) % n
        assert _same_bits(_solve(device, pc.take(c, idx)), ref[idx]), N
    filler = pc.good_rows(1, npts)
    fill_ref = _solve(device, filler)[0]
    both = pc.concat(c, filler)  # row n = the filler

    def batch_of_300(where):
        """Rows ``where[p]`` (index into c, -1 = filler) at position p, solved as one batch of 300."""
        where = np.asarray(where)
        assert where.shape == (300,)
        idx = np.where(where < 0, n, where)
        out = _solve(device, pc.take(both, idx))
        want = np.where((where >= 0)[:, None], ref[np.clip(where, 0, n - 1)], fill_ref[None, :])
        return _same_bits(out, want), out

    for off in range(4):  # every lane quarter of a wavefront
        where = np.full(300, -1)
        where[4 * np.arange(n) + off] = np.arange(n)
        ok, out = batch_of_300(where)
        assert ok, ("offset", off)
        if off == 0:
            ok, _ = batch_of_300(where[::-1].copy())  # reversed order
            assert ok, "reversed"
    # next to every kind of neighbour: the three other detections of the wavefront are copies of one representative
    kinds = {}
    for i in range(n):
        nv = int((c.pts[i] > -5000).all(axis=1).sum())
        kinds.setdefault((st[i], "epnp" if 4 <= nv < 6 else "planar" if "planar" in c.names[i] else "nan" if not np.isfinite(c.pts[i]).all() else ""), i)
    assert len(kinds) >= (8 if npts == 16 else 3), kinds
    for kind, k in kinds.items():
        for chunk in range(0, n, 70):
            js = np.arange(chunk, min(n, chunk + 70))
            where = np.full(300, -1)
            where[: 4 * len(js)] = k
            where[4 * np.arange(len(js)) + 1] = js
            ok, _ = batch_of_300(where)
            assert ok, ("neighbour", kind, c.names[k])


@pytest.mark.parametrize("kind", ["planar", "five_points"])
def test_rare_list_with_every_row_rare(device, kind):
    """N = 300, every row on pnp_rare_kernel's list (appended with atomicAdd, in whatever order the groups arrive): rows equal
    the same rows solved in two batches of 150 (one workgroup per detection), and two runs are bit-identical."""
    c = pc.planar_rows(300) if kind == "planar" else pc.five_point_rows(300)
    out = _solve(device, c)
    assert set(out[:, 0]) <= {0.0, 1.0, 2.0} and (out[:, 0] == 1).sum() >= 150  # (well-posed rows: most have a pose)
    assert (out[:, 35] == (8 if kind == "planar" else 5)).all()
    solved = out[:, 0] >= 1
    assert (out[solved, 36] > 0).all() if kind == "planar" else (out[:, 36] == 0).all()  # LM after the homography, none after EPnP
    small = np.concatenate([_solve(device, pc.take(c, range(0, 150))), _solve(device, pc.take(c, range(150, 300)))])
    assert _same_bits(out, small)
    assert _same_bits(_solve(device, c), out)
    for i in np.where(out[:, 0] == 1)[0][:40]:
        _self_consistent(out[i], c.pts[i], c.scale[i], c.cam[i])


def test_pnp_from_post_above_256_slots(device):
    """B = 3, K = 100 (300 slots: four detections per wavefront), count = [100, 37, 0]: test_pnp_from_post_assembly_by_value's
    check at that size -- rows bit-identical to cp_pnp_solve on host-assembled points, status -1 past count[b]."""
    from tests.test_gpu_pose_chain import CAM4, _posed_records, _reference_points

    B, K, counts = 3, 100, [100, 37, 0]
    cam = np.array([[CAM4[0] * (1 + 0.01 * b), CAM4[1] * (1 - 0.01 * b), CAM4[2] + b, CAM4[3] - b] for b in range(B)])
    post, _ = _posed_records(B, K, counts, 77, cam)
    out = hip.pnp_from_post(torch.from_numpy(post).to(device), torch.tensor(counts, dtype=torch.int32, device=device),
                            torch.from_numpy(cam).to(device), rep_mode=1).cpu().numpy()
    assert out.shape == (B, K, hip.PNP_STRIDE)
    for b in range(B):
        assert (out[b, counts[b]:, 0] == -1).all()
        if counts[b] == 0:
            continue
        pts = np.stack([_reference_points(post[b, k], 1) for k in range(counts[b])]).astype(np.float32)
        host = hip.pnp_solve(torch.from_numpy(pts).to(device),
                             torch.from_numpy((post[b, :counts[b], 2:5] / post[b, :counts[b], 3:4]).astype(np.float32)).to(device),
                             torch.from_numpy(np.tile(cam[b], (counts[b], 1))).to(device)).cpu().numpy()
        assert (host[:, 0] >= 1).all()
        assert _same_bits(out[b, :counts[b]], host), b


def test_useless_inputs(device):
    """NaN / Inf image points, zero / NaN / negated sizes, a zero focal length, a NaN principal point, mirrored images: the call
    returns, every status is defined, a status-1 row is finite and consistent with its own pose, rows the oracle has an
    answer for match it, and the good rows that share a wavefront with the bad ones do not change by a bit."""
    c = pc.useless_inputs()
    out = _solve(device, c)
    rows = pc.oracle_rows(c)
    print("\nstatus per row:", {nm: int(s) for nm, s in zip(c.names, out[:, 0])})
    assert set(out[:, 0]) <= {-1.0, 0.0, 1.0, 2.0}
    for i, (nm, r) in enumerate(zip(c.names, rows)):
        if out[i, 0] == 1:
            _self_consistent(out[i], c.pts[i], c.scale[i], c.cam[i])
        else:
            assert np.isfinite(out[i]).all(), nm
        if nm in pc.USELESS_UNDERDETERMINED or r.kind == "undefined":
            continue
        if r.kind == "none":
            assert r.why == "behind_camera" and out[i, 0] == 2, nm
            continue
        assert out[i, 0] == 1, nm
        d = pc.pose_diff(pc.device_pose(out[i]), r)
        assert all(d[q] <= pc.BASE_LIMITS[q] for q in pc.QUANTITIES) and int(out[i, 36]) == r.iters, (nm, d)
    i = c.index["one coordinate -Inf"]
    assert out[i, 0] == 1 and out[i, 35] == 15  # below -5000: dropped, the row stays solvable
    # N = 300: bad row k at position 4 k + (k mod 4), its wavefront's other three detections (and everything else) good
    n = len(c.names)
    good = pc.good_rows(300)
    both = pc.concat(good, c)
    idx = np.arange(300)
    pos = np.array([4 * k + k % 4 for k in range(n)])
    idx[pos] = 300 + np.arange(n)
    mixed = _solve(device, pc.take(both, idx))
    clean = _solve(device, good)
    keep = np.ones(300, bool)
    keep[pos] = False
    assert (clean[:, 0] >= 1).all()
    assert _same_bits(mixed[keep], clean[keep])
    assert _same_bits(mixed[pos], out)
