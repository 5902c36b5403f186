"""No GPU: the restatements of tests/neighbors3d_cases.py against their pure-Python all-pairs definitions and against
scipy's anisotropic distance transform, the consequences the header states, the new argument checks of
sequitr_amd/analysis/neighbors.py, and SERVER_segment_volume's early refusals of the measure / neighbours options."""
import os

import numpy as np
import pytest
from scipy import ndimage

from sequitr_amd import jobs
from sequitr_amd.analysis import neighbors as nb
from tests import neighbors3d_cases as n3
from tests import neighbors_cases as nc


@pytest.mark.parametrize("case", n3.small_cases(), ids=lambda c: c[0])
def test_zones_restatement_equals_the_all_pairs_definition(case):
    name, lab, ml = case
    assert lab.shape[1:] <= (4, 5, 6)
    planar = n3.planar_ref(lab, ml)
    for dz in n3.EXACT_DZS:
        for R in (0, 2):
            z, d = n3.zones3d_from_planar(*planar, dz=dz, max_distance=R)
            za, da = n3.zones3d_allpairs(lab, ml, R, dz)
            assert z.dtype == np.int32 and d.dtype == np.float64
            assert np.array_equal(z, za) and np.array_equal(d.view(np.uint64), da.view(np.uint64)), (name, dz, R)


def test_the_tie_cases_hold_the_ties_they_are_built_for():
    for name, lab, ml, _, _ in n3.tie_cases():
        a, b = int(name[-2]), int(name[-1])
        z, d = n3.zones3d_ref(lab, ml)
        assert [d[n, 5, 3, 5] for n in range(4)] == [1.0, 9.0, 25.0, 25.0], name
        assert [int(z[n, 5, 3, 5]) for n in range(4)] == [1, 1, 1, 1], name          # the smaller label, whichever is met first
        assert {a, b} == {1, 2}
    # volume 3 is the tie only the A(k) <= best continuation finds: A(5) == 9 + 16, the smaller label at P == 0
    lab = n3.tie_cases()[1][1]
    assert lab[3, 8, 3, 9] == 2 and lab[3, 0, 3, 5] == 1 and n3.depth_term(5, 1.0) == 25.0


def test_the_stated_consequences_hold():
    for name, lab, ml, reaches, dzs in n3.shape_cases()[:6] + n3.empty_cases() + n3.volume_leak_cases():
        planar = n3.planar_ref(lab, ml)
        seeds = nc.seeds_of(lab, ml)
        has_seed = seeds.reshape(len(lab), -1).any(1)
        for dz in dzs:
            z, d = n3.zones3d_from_planar(*planar, dz=dz)
            assert np.array_equal(z[seeds > 0], seeds[seeds > 0]), (name, dz)       # a seed lies in its own zone
            assert np.all(z[has_seed] > 0) and not z[~has_seed].any()               # zones cover a volume with a seed
            assert np.all(np.isinf(d[~has_seed])) and np.all(np.isfinite(d[has_seed]))
            again = n3.zones3d_from_planar(*planar, dz=dz)
            assert np.array_equal(z, again[0]) and np.array_equal(d, again[1])
            for R in reaches:
                if R:
                    zr, dr = n3.zones3d_from_planar(*planar, dz=dz, max_distance=R)
                    assert np.array_equal(dr.view(np.uint64), d.view(np.uint64))
                    assert np.array_equal(zr, np.where(d <= float(R * R), z, 0))
    # nothing leaks between volumes: a volume's zones are those of the volume on its own
    name, lab, ml, _, _ = n3.volume_leak_cases()[0]
    whole = n3.zones3d_ref(lab, ml)
    for n in range(3):
        alone = n3.zones3d_ref(lab[n:n + 1], ml)
        assert np.array_equal(whole[0][n], alone[0][0]) and np.array_equal(whole[1][n], alone[1][0])


def test_reach_keeps_the_boundary_and_drops_the_next_value():
    name, lab, ml, reaches, _ = n3.reach_case()
    _, d = n3.zones3d_ref(lab, ml)
    assert d[0, 4, 2, 6] == 64.0 ** 2 and d[0, 3, 2, 6] == 64.0 ** 2 + 1 and d[0, 1, 2, 74] == 25.0 and d[0, 1, 3, 74] == 26.0
    for R, kept, dropped in ((64, (4, 2, 6), (3, 2, 6)), (5, (1, 2, 74), (1, 3, 74)), (1, (4, 2, 71), (3, 2, 71))):
        z, _ = n3.zones3d_ref(lab, ml, R)
        assert z[(0,) + kept] == 2 and z[(0,) + dropped] == 0, R


@pytest.mark.parametrize("dz", n3.EXACT_DZS)
def test_d2_of_the_restatement_is_scipys_anisotropic_transform(dz):
    for name, lab, ml, _, _ in n3.shape_cases()[1:7] + [n3.seam_case()]:
        _, d = n3.zones3d_ref(lab, ml, dz=dz)
        seeds = nc.seeds_of(lab, ml)
        for n in range(len(lab)):
            if seeds[n].any():
                want = ndimage.distance_transform_edt(seeds[n] == 0, sampling=(dz, 1, 1)) ** 2
                # scipy squares a square root: equal up to that rounding, and exactly once rounded back to the lattice
                assert np.array_equal(np.round(want * 4), d[n] * 4), (name, dz, n)


@pytest.mark.parametrize("case", n3.graph_cases()[:4] + [n3.random_zones(5, 2, 3, 4, 9, 4)], ids=lambda c: c[0])
def test_graph_restatement_equals_the_all_pairs_definition(case):
    name, z, ml = case
    s, p = n3.graph3d_ref(z, ml)
    sa, pa = n3.graph3d_allpairs(z, ml)
    assert np.array_equal(s, sa) and np.array_equal(p, pa), name
    assert p.shape[1] == 5 and np.all(p[:, 1] < p[:, 2]) and np.all(p[:, 3] + p[:, 4] > 0)


def test_graph_cases_separate_lateral_from_axial():
    (_, lat, _), (_, axi, _) = n3.plane_borders()
    assert n3.graph3d_ref(lat, 2)[1].tolist() == [[0, 1, 2, 3 * 70, 0]]
    assert n3.graph3d_ref(axi, 2)[1].tolist() == [[0, 1, 2, 0, 3 * 70]]
    name, z, ml = n3.l_shaped_two_volumes()
    s, p = n3.graph3d_ref(z, ml)
    both = p[(p[:, 1] == 1) & (p[:, 2] == 2)]
    assert both[:, 0].tolist() == [0, 1] and np.all(both[0, 3:] > 0)              # the same pair in two volumes
    assert both[1].tolist() == [1, 1, 2, 0, 6]
    assert not ((p[:, 1] == 2) & (p[:, 2] == 3)).any()                            # zone 0 lies between them
    assert s[0, 4].tolist() == [7, 7]                                             # a corner and an edge run: once each
    assert len(n3.graph3d_ref(n3.five_pairs()[1], 6)[1]) == 5


def test_check_params_refuses_bad_values_of_the_new_keys():
    assert nb.check_params(50, 7, "centroids", 2.5) == (50.0, 7, "centroids", 2.5)
    assert nb.check_params(50, 7, "centroids") == (50.0, 7, "centroids")          # the planar form is what it was
    assert nb.check_spacing(1) == 1.0 and isinstance(nb.check_spacing(np.float32(0.5)), float)
    for bad in (0, -1.0, float("nan"), float("inf"), "wide", True, [1.0]):
        with pytest.raises(ValueError, match="spacing"):
            nb.check_params(spacing=bad)
        with pytest.raises(ValueError, match="spacing"):
            nb.check_spacing(bad)
    with pytest.raises(ValueError, match="spacing"):
        nb.check_spacing(None)
    with pytest.raises(ValueError, match="d_thresh"):
        nb.check_params(-1.0, spacing=2.0)
    with pytest.raises(ValueError, match="seeds"):
        nb.check_params(seeds="voxels", spacing=2.0)


def test_planar_tables_keep_their_columns_and_volumetric_ones_add_three():
    stats = np.zeros((1, 3, 2), np.int64)
    stats[0, 1], stats[0, 2] = (10, 4), (6, 6)
    flat = nb.NeighborTable([0, 0], [1, 2], [1, 1], np.array([[0., 0., 0.], [0., 3., 4.]]), 2, stats, [[0, 1, 2, 7]], 1)
    assert not flat.volumetric and tuple(flat.columns()) == nc.TABLE_COLUMNS and flat.border.tolist() == [7, 7]
    assert flat.distance.tolist() == [5.0, 5.0] and flat.local_density.tolist() == [0.1, 1.0 / 6.0]
    vol = nb.NeighborTable([0, 0], [1, 2], [1, 1], np.array([[1., 0., 0.], [3., 3., 0.]]), 2, stats, [[0, 1, 2, 7, 2]], 1,
                           volumetric=True, spacing=2.0)
    assert vol.volumetric and tuple(vol.columns()) == n3.TABLE_COLUMNS
    assert vol.distance.tolist() == [5.0, 5.0]                                    # sqrt((2 * 2)^2 + 3^2)
    assert vol.border.tolist() == [9, 9] and vol.border_lateral.tolist() == [7, 7] and vol.border_axial.tolist() == [2, 2]
    assert vol.contact_area.tolist() == [16.0, 16.0] and vol.contact_area.dtype == np.float64
    assert vol.local_density.tolist() == [1.0 / 20.0, 1.0 / 12.0] and vol.zone_edge.tolist() == [4, 6]
    far = nb.NeighborTable([0, 0], [1, 2], [1, 1], np.array([[1., 0., 0.], [3., 3., 0.]]), 2, stats, [[0, 1, 2, 7, 2]], 1,
                           d_thresh=4.9, volumetric=True, spacing=2.0)
    assert far.n_pairs == 0 and far.n_removed.tolist() == [1, 1]
    cat = nb.NeighborTable.concatenate([vol, vol], [0, 1], 2)
    assert cat.volumetric and cat.spacing == 2.0 and cat.frame.tolist() == [0, 0, 1, 1] and cat.indices.tolist() == [1, 0, 3, 2]
    want = {k: np.concatenate([v, v]) for k, v in vol.columns().items()}
    want.update(frame=cat.frame, indices=cat.indices, indptr=np.array([0, 1, 2, 3, 4]))
    n3.assert_table(cat.columns(), want, "concatenate")
    flat2 = nb.NeighborTable.concatenate([flat, flat], [0, 1], 2)
    assert not flat2.volumetric and tuple(flat2.columns()) == nc.TABLE_COLUMNS
    with pytest.raises(ValueError, match="all planar or all volumetric"):
        nb.NeighborTable.concatenate([flat, vol], [0, 1], 2)


class _Untouchable(np.ndarray):
    """an array whose voxels must not be touched: the job under test raises before it reads one"""

    def __getitem__(self, key):
        raise AssertionError("the job read the input")


OPTIONS = ("measure", "save_labels", "neighbors", "save_zones")


def test_segment_volume_refuses_the_options_without_brick_before_any_input_is_opened(tmp_path):
    vols = np.zeros((2, 4, 8, 8), np.uint16).view(_Untouchable)
    for src in (str(tmp_path / "missing.npy"), vols):            # an input that does not even exist
        for opt in OPTIONS:
            with pytest.raises(ValueError, match="brick"):
                jobs.SERVER_segment_volume({"input": src, "output": str(tmp_path)}, {opt: True})
    assert os.listdir(str(tmp_path)) == []


def test_segment_volume_refuses_bad_neighbour_parameters_before_any_input_is_opened(tmp_path):
    vols = np.zeros((2, 4, 8, 8), np.uint16).view(_Untouchable)
    for src in (str(tmp_path / "missing.npy"), vols):
        base = {"input": src, "output": str(tmp_path), "brick": (8, 8, 4)}
        for bad, match in (({"spacing": 0}, "spacing"), ({"spacing": "thick"}, "spacing"), ({"spacing": float("nan")}, "spacing"),
                           ({"d_thresh": -1}, "d_thresh"), ({"d_thresh": "far"}, "d_thresh"),
                           ({"neighbor_seeds": "voxels"}, "seeds"), ({"zone_reach": 0}, "max_distance"),
                           ({"zone_reach": 2.5}, "max_distance")):
            for opts in ({"neighbors": True}, {"neighbors": True, "measure": True, "save_zones": True}):
                with pytest.raises(ValueError, match=match):
                    jobs.SERVER_segment_volume(dict(base, **bad), opts)
        with pytest.raises(ValueError, match="min_area"):
            jobs.SERVER_segment_volume(dict(base, min_area=5, max_area=4), {"measure": True})
    assert os.listdir(str(tmp_path)) == []
