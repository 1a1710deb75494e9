"""The reference helpers behind tests/test_probes_edges_gpu.py, without a GPU: probe_ref.sample's callable volume against the array;
hashed_volume built with torch against its numpy records; every named row of probe_edges holding the edge it claims - a subnormal
wsum, an exact-zero wsum of non-zero weights, non-finites behind a zero validity with a finite result, 0 * inf counting; the share
of the edge set that the NaN rule covers; the seed products of the points at the axis limit passing 2^32; the NaN rule's helper."""
import warnings

import numpy as np
import pytest

import probe_edges as E
import probe_ref as P

U, F = np.uint32, np.float32
COUNTS = [(1, 1, 1), (2, 1, 1), (1, 3, 1), (2, 2, 2), (5, 4, 3)]
GRID = dict(origin=(0.5, -1.0, 2.0), spacing=(0.5, 0.25, 1.5))


def bits(a):
    return np.ascontiguousarray(a, F).view(U)


def test_this_process_keeps_denormals():
    """The reference is worth nothing at the subnormal rows if something this process loaded made the CPU flush them."""
    tiny = np.array([1e-45, 1.17549435e-38], F)
    assert (tiny * F(1) != 0).all() and (tiny[1:] * F(0.5) != 0).all()
    assert F(4e-42) / F(2e-42) == F(2.0)


@pytest.mark.parametrize("count", COUNTS)
def test_sample_takes_a_callable(count):
    d = P.desc(GRID["origin"], GRID["spacing"], count)
    vol = P.fabricated_volume(count, 9)
    flat = vol.reshape(-1, 28)
    pts = P.sample_points(d, 260, 5, nonfinite=True)
    seen = []

    def records(q):
        assert q.dtype == np.int64 and q.ndim == 1
        seen.append(q)
        return flat[q]
    want = P.sample(d, vol, pts)
    got = P.sample(d, records, pts)
    assert (bits(got) == bits(want)).all() and len(seen) == 8
    assert np.concatenate(seen).max() == len(flat) - 1 and np.concatenate(seen).min() == 0
    out, w, wsum, q = P.sample(d, vol, pts, detail=True)
    assert (bits(out) == bits(want)).all() and w.shape == (260, 8) and (q == np.stack(seen, 1)).all()
    assert (bits(np.where(wsum == 0, F(0), wsum)) == bits(want[:, 3])).all()


def test_hashed_volume_by_torch_and_by_numpy():
    count = (5, 4, 3)
    vol = P.hashed_volume(count, "cpu", slab=7).numpy()               # (nine slabs, the last ragged)
    assert vol.shape == (3, 4, 5, 28) and vol.dtype == F
    rec = P.hashed_records(np.arange(60))
    assert (bits(vol.reshape(60, 28)) == bits(rec)).all()
    assert (bits(P.hashed_volume(count, "cpu").numpy()) == bits(vol)).all()
    valid = rec[:, 27]
    assert set(np.unique(valid).tolist()) == {0.0, 0.25, 1.0}, np.unique(valid)
    assert not np.isfinite(rec[valid == 0, 0:27]).any() and np.isnan(rec[valid == 0, 0]).all() and np.isinf(rec[valid == 0, 1]).all()
    live = rec[valid != 0, 0:27]
    assert np.isfinite(live).all() and live.min() >= -1 and live.max() < 1 and len(np.unique(live)) > 0.99 * live.size
    # 24 bits a coefficient: a multiple of 2^-23, so the float32 steps were exact
    assert (live.astype(np.float64) * 2.0 ** 23 % 1 == 0).all()
    # the far end of the index range: p * 28 + k stays below 2^27 and the classes still occur
    far = P.hashed_records(np.arange((1 << 22) - 4096, 1 << 22))
    assert [int((far[:, 27] == v).sum()) > 512 for v in (0.0, 0.25, 1.0)] == [True] * 3
    assert (bits(far[-1:]) == bits(P.hashed_records([(1 << 22) - 1]))).all() and (bits(far[-1]) != bits(far[-2])).any()


def test_points_of_a_grid_that_overflows_come_without_warnings():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = {name: P.points(d) for name, d in E.point_grids()}
    first = got["origin 3e38, spacing 3e38: positions overflow to +inf"]
    assert first[0, 0:3].tolist() == [F(3e38)] * 3 and np.isposinf(first[1, 0]) and np.isposinf(first[-1, 0:3]).all()
    assert (got["origin -3e38, ordinary spacing"][:, 0:3] == F(-3e38)).all()           # (the spacing is absorbed)
    assert got["origin -3e38, spacing 3e38"][-1, 0:3].tolist() == [np.inf, 0.0, 0.0]       # (-3e38 + 2 * 3e38: the product alone overflows)
    tiny = got["spacing 1e-45 at count 3"]
    assert bits(tiny[:3, 0]).tolist() == [0, 1, 2] and (tiny[:, 1] == -1).all()


@pytest.mark.parametrize("count", E.AXIS_LIMIT)
def test_seed_products_pass_two_to_the_32(count):
    d = P.desc((-1.25, 0.5, 3.0), (0.3, 0.7, 0.011), count, E.WRAP_SEED, E.WRAP_STRIDE)
    pts = P.points(d)
    n = count[0] * count[1] * count[2]
    assert (n - 1) * E.WRAP_STRIDE >> 32 >= 632 and 2 * E.WRAP_STRIDE >= 1 << 32
    assert bits(pts)[:, 6].tolist() == [(E.WRAP_SEED + p * E.WRAP_STRIDE) % (1 << 32) for p in range(n)]
    # neither the full product nor a float product gives these words
    assert bits(pts)[2, 6] != (E.WRAP_SEED + 2 * E.WRAP_STRIDE) % (1 << 64) and len(set(bits(pts)[:, 6].tolist())) == n


def test_the_nan_rule_helper():
    want = np.array([[1.0, np.nan, -0.0, 0.0]], F)
    nan2 = np.array([0xFFC00001], U).view(F)[0]                          # another sign, another payload
    assert E.assert_bits_or_nan(np.array([[1.0, nan2, -0.0, 0.0]], F), want, "x") == 1
    assert E.assert_bits_or_nan(want[:, [0, 2]], want[:, [0, 2]], "x") == 0
    for bad in ([1.0, 5.0, -0.0, 0.0], [1.0, np.nan, 0.0, 0.0], [np.nan, np.nan, -0.0, 0.0], [1.0, np.inf, -0.0, 0.0]):
        with pytest.raises(AssertionError) as e:
            E.assert_bits_or_nan(np.array([bad], F), want, "the case", names=["the row"])
        assert "the case" in str(e.value) and "record 0 (the row)" in str(e.value) and "words [" in str(e.value)


def _group(count, grid, volume):
    found = [g for g in E.edge_cases() if g["name"].startswith(f"{count}, {grid}; {volume}")]
    assert len(found) == 1, (count, grid, volume, [g["name"] for g in found])
    return found[0]


def _row(g, start):
    found = [i for i, n in enumerate(g["names"]) if n.startswith(start)]
    assert len(found) == 1, (start, g["names"])
    return found[0]


def test_the_edge_set_names_every_edge():
    names = [g["name"] for g in E.edge_cases()]
    assert len(set(names)) == len(names)
    for count in E.COUNTS:
        gn = [n for n, _ in E.grids(count)]
        assert len(gn) == 12 and all(any(n.startswith(f"{count}, {k};") for n in names) for k in gn)
        vn, vols = E.edge_volume(count)
        assert vols.shape == (len(vn), count[0] * count[1] * count[2], 28)
        assert all(any(n == f"{count}, ordinary; {k}" for n in names) for k in vn)
    nn, normals = E.edge_normals()
    assert len(nn) == 14 and (normals[0] == 0).all() and np.signbit(normals[1]).all() and np.isnan(normals[2]).any() and np.isinf(normals[3]).any()
    for g in E.edge_cases():
        assert len(g["names"]) == len(g["pts"]) and not g["pts"].flags.writeable and not g["volume"].flags.writeable
    # both routes have rows at every group but none: the host route's share
    share = [int(E.host_route(g["pts"]).sum()) for g in E.edge_cases()]
    assert min(share) >= 9, share


def test_positions_sit_where_their_names_say():
    """one ulp either side of a plane lands in the cell below and the cell above (the reference's own i0 and f)"""
    for count in E.COUNTS:
        d = dict(E.grids(count))["ordinary"]
        names, pts = E.edge_points(d)
        for a in range(3):
            m = count[a] - 1
            i0, i1, w0, w1 = P.axis(pts[:, a], d["origin"][a], d["spacing"][a], count[a])
            for i in range(count[a]):
                lo, on, hi = (names.index(f"axis {a}: {t} plane {i}") for t in ("one ulp below", "on", "one ulp above"))
                assert w1[on] == (1.0 if i == m and m > 0 else 0.0) and i0[on] == min(i, max(m - 1, 0)), (count, a, i)
                if 0 < i:
                    assert i0[lo] == i - 1 and 0.999 < w1[lo] < 1, (count, a, i, w1[lo])
                if i < m:
                    assert i0[hi] == i and 0 < w1[hi] < 1e-5, (count, a, i, w1[hi])
            k = names.index(f"axis {a}: the float below the origin")
            assert pts[k, a] < d["origin"][a] and w1[k] == 0 and i0[k] == 0
    for count in E.COUNTS:
        for gname, d in E.grids(count):
            names, pts = E.edge_points(d)
            for a in range(3):
                with np.errstate(over="ignore", invalid="ignore"):
                    diff = pts[:, a] - d["origin"][a]
                if gname == f"spacing[{a}] 1e-45":
                    k = names.index(f"axis {a}: -0.0 before an origin of +0.0")
                    assert diff[k] == 0 and np.signbit(diff[k])                                  # a difference of -0.0
                    k = names.index(f"axis {a}: the float below the origin")
                    assert diff[k] < 0 and abs(diff[k]) < E.MIN_NORMAL                           # a negative subnormal
                if gname.startswith("origin"):
                    k = names.index(f"axis {a}: the opposite extreme (pos - origin overflows)")
                    assert np.isfinite(pts[k, 0:6]).all() and np.isinf(diff[k])


def test_subnormal_rows_divide_subnormals():
    """spacing 3e38, 1e-3 behind the origin, the near plane invalid: the far corner's weight is f itself, about 3.3e-42, wsum with
    it - non-zero and below the least normal float, so a reference that flushed would fail here - and the result is the far probes'
    finite irradiance."""
    seen = 0
    for count in E.COUNTS:
        for a in range(3):
            if count[a] < 2:
                continue
            g = _group(count, f"spacing[{a}] 3e38", f"plane 0 of axis {a} invalid")
            k = _row(g, f"axis {a}: a subnormal f")
            out, w, wsum, q = P.sample(g["d"], g["volume"], g["pts"], detail=True)
            assert 0 < wsum[k] < E.MIN_NORMAL and out[k, 3] == wsum[k], (g["name"], wsum[k])
            assert 3e-42 < wsum[k] < 4e-42 and (w[k] != 0).sum() == 1 and np.isfinite(out[k]).all() and (out[k, 0:3] != 0).all()
            # the quotient of subnormals gave the far probe's record back: 2353 steps of 1e-45 in f, so to about 1 part in 2000
            far = g["volume"][q[k][w[k] != 0][0]]
            alone = P.sample(g["d"], np.repeat(far[None], len(g["volume"]), 0), g["pts"][k:k + 1])
            assert np.abs(out[k, 0:3] - alone[0, 0:3]).max() <= 2e-3 * np.abs(far[0:27]).max() * 9
            seen += 1
    assert seen == 5


def test_value_rows_hold_what_they_claim():
    for count in E.COUNTS:
        def run(volume):
            g = _group(count, "ordinary", volume)
            return (g,) + P.sample(g["d"], g["volume"], g["pts"], detail=True)
        # wsum exactly 0 from two weights that are not
        g, out, w, wsum, q = run(E.CANCEL)
        k = _row(g, E.MIDWAY)
        assert sorted(w[k][w[k] != 0].tolist()) == [-0.5, 0.5] and wsum[k] == 0 and not np.signbit(wsum[k]) and (bits(out[k]) == 0).all()
        assert np.isfinite(out).all(), "+-inf behind a zero validity leaked"
        # non-finites behind a zero validity of either sign: a finite result at every row
        for volume in ("+-inf coefficients behind a zero validity", "validity -0.0", "mixed validity"):
            g, out, w, wsum, q = run(volume)
            assert np.isfinite(out).all() and not np.isfinite(g["volume"][g["volume"][:, 27] == 0, 0:27]).any(), volume
            assert (w == 0).any() and not np.isfinite(g["volume"][q[w == 0]]).all()
        g, out, w, wsum, q = run("validity -0.0")
        assert np.signbit(g["volume"][0, 27]) and (np.signbit(w) & (w == 0)).any()
        # a subnormal validity: weights and their products with the coefficients are subnormal where probe 0 stands alone
        g, out, w, wsum, q = run("validity subnormal")
        sub = (w != 0) & (np.abs(w) < E.MIN_NORMAL)
        assert sub.any() and np.isfinite(out).all()
        # 0 * inf is a NaN that counts
        for volume in ("validity +inf on probe 1", "validity -inf on probe 1"):
            g, out, w, wsum, q = run(volume)
            k = _row(g, "the origin")
            assert q[k, 1] == 1 and np.isnan(w[k, 1]) and np.isnan(out[k]).all(), (volume, w[k], out[k])
            assert np.isinf(w).any()
        g, out, w, wsum, q = run("validity NaN")
        assert np.isnan(out[_row(g, "the origin")]).all() and np.isfinite(out).all(1).any()
        g, out, w, wsum, q = run("validity 3e38")
        assert np.isinf(out[:, 0:3]).any() or np.isnan(out[:, 0:3]).any()
        assert np.isfinite(out[:, 3]).all() and out[:, 3].max() > 1e38
        # non-finite and huge coefficients behind a valid probe propagate
        g, out, w, wsum, q = run("coefficients 3e38 behind a valid probe")
        assert np.abs(out[_row(g, "the origin"), 0:3]).max() > 1e37 and np.isfinite(out[:, 3]).all()
        g, out, w, wsum, q = run("+-inf coefficients behind a valid probe")
        assert not np.isfinite(out[_row(g, "the origin"), 0:3]).any() and np.isfinite(out[:, 3]).all()


def test_normal_rows_hold_what_they_claim():
    g = [g for g in E.edge_cases() if g["name"].endswith("the normals")][0]
    out = P.sample(g["d"], g["volume"], g["pts"])
    by = dict(zip(g["names"], out))
    assert (bits(out[:, 3]) == bits(out[0, 3])).all() and out[0, 3] == 1.0                 # wsum intact at every row
    for name in ("all zero", "all -0.0", "a NaN component", "an infinite component", "length 1e-42, one component", "length 1e-30, one component",
                 "length 1e-42, two components", "length 1e-30, two components"):
        assert np.isnan(by[name][0:3]).all(), (name, by[name])
    for name in ("length 1e-20, one component", "length 1e-20, two components", "length 1e19, one component", "length 1e19, two components",
                 "length 3e30, one component", "length 3e30, two components"):
        assert np.isfinite(by[name]).all() and (by[name][0:3] != 0).all(), (name, by[name])
    # 1e-20 and 1e19 normalise to the unit vector's result to a few ulps; 3e30 overflows to a zero vector: the constant band alone
    unit = g["pts"][[8]].copy()
    unit[0, 3:6] = (0, 1, 0)
    assert np.allclose(by["length 1e-20, one component"], P.sample(g["d"], g["volume"], unit)[0], rtol=1e-5)
    assert np.allclose(by["length 1e19, one component"], P.sample(g["d"], g["volume"], unit)[0], rtol=1e-5)
    assert (bits(by["length 3e30, one component"]) == bits(by["length 3e30, two components"])).all()


def test_the_nan_rule_covers_under_a_quarter():
    rows = covered = 0
    for g in E.edge_cases():
        out = P.sample(g["d"], g["volume"], g["pts"])
        rows += len(out)
        covered += int(np.isnan(out).any(1).sum())
    print(f"{covered} of {rows} rows hold a NaN word in the reference")
    assert rows > 1000 and 0 < covered <= rows // 4


def test_size_edge_points_reach_both_ends():
    """the long-axis and probe-limit point sets: the first, a middle and the last cell of every axis, the named planes, index n - 1"""
    for count in E.LONG_AXES + E.PROBE_LIMIT:
        d = P.desc(GRID["origin"], GRID["spacing"], count)
        pts = E.limit_points(d, 3)
        assert len(pts) == E.N_LONG + 18 + 27
        n = count[0] * count[1] * count[2]
        a = int(np.argmax(count))
        i0, i1, w0, w1 = P.axis(pts[:, a], d["origin"][a], d["spacing"][a], count[a])
        assert {0, 1, 254, 255, 256, 1021, 1022} <= set(i0.tolist()) and i1.max() == 1023
        q = ((P.axis(pts[:, 2], d["origin"][2], d["spacing"][2], count[2])[1] * count[1]
              + P.axis(pts[:, 1], d["origin"][1], d["spacing"][1], count[1])[1]) * count[0] + P.axis(pts[:, 0], d["origin"][0], d["spacing"][0], count[0])[1])
        assert q.max() == n - 1
        for b in range(3):
            j0 = P.axis(E.cell_points(d)[:, b], d["origin"][b], d["spacing"][b], count[b])[0]
            assert set(j0.tolist()) == {0, max(count[b] - 1, 1) // 2, max(count[b] - 2, 0)}, (count, b)
