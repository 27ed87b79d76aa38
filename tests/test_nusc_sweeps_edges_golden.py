"""The sweep merger at its edges, against the reference's recorded results (tests/golden/nusc_sweeps_edges.npz, made by
tools/make_golden.py --only sweeps_edges from the scenarios of tests/nusc_sweeps_edges_common.py): the host form, the
coverage the GPU test relies on, and the device kernel's contract evaluated with numpy."""
import os

import numpy as np
import pytest

import fake_nuscenes as fk
import nusc_sweeps_edges_common as ec
from conftest import GOLDEN


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(GOLDEN, 'nusc_sweeps_edges.npz'), allow_pickle=False)


def check_result(out, want):
    assert out['points'].dtype == np.float32 and out['points'].shape == want['points'].shape
    assert np.array_equal(out['points'], want['points'])
    assert list(out['instances_token']) == list(want['instances_token'])
    assert np.array_equal(np.stack(out['instances_center']), want['instances_center'])
    assert np.array_equal(out['instances_last_box'], want['instances_last_box'])
    assert np.array_equal(out['instances_name'], want['instances_name'])


def fake(fixture, scenario, tmp_path):
    return fk.FakeNuScenes(ec.load_tables(fixture, scenario), tmp_path, quaternion=lambda q: np.asarray(q))


@pytest.mark.parametrize('scenario', sorted(ec.SCENARIOS))
def test_host_merger_matches_reference_at_the_edges(fixture, scenario, tmp_path):
    from datasets.nuscenes_sweeps import inst_centric_get_sweeps
    out = inst_centric_get_sweeps(fake(fixture, scenario, tmp_path), 'sample0', **ec.cfg(scenario))
    check_result(out, ec.expected(fixture, scenario))


def test_generator_is_the_fixture(fixture):
    """the committed tables are what the generator makes (the coverage below is a property of the generator)"""
    for scenario in ec.SCENARIOS:
        made, stored = ec.TABLES[scenario](), ec.load_tables(fixture, scenario)
        assert set(made) == set(stored)
        for key in made:
            if key == 'points':
                assert all(np.array_equal(a, b) for a, b in zip(made[key], stored[key]))
            else:
                assert np.array_equal(np.asarray(made[key]), stored[key]), key


def test_coverage_scenario_a(fixture):
    """per record: at least 200 face points labelled and 200 unlabelled, at least 50 circle points kept and 50 dropped"""
    cov = ec.coverage_a(ec.load_tables(fixture, 'a'), fixture['a_points'])
    print('face labelled / unlabelled, circle kept / dropped per record:', cov)
    assert len(cov) == 3
    for lab, unlab, kept, dropped in cov:
        assert lab >= 200 and unlab >= 200 and kept >= 50 and dropped >= 50


def test_coverage_scenario_b(fixture):
    """empty file, sweep without candidate box, 512 / 511 / 513 kept points, labelled rows in lanes 0 and 63 and in the
    first and last row of a tile, overlapping boxes, a track opened by a later box"""
    t, p = ec.load_tables(fixture, 'b'), fixture['b_points']
    assert t['points'][0].shape[0] == 0 and not (t['box_lidar_pts'][t['box_record'] == 1] > 0).any()
    assert [int((p[:, 5] == k).sum()) for k in range(4)] == list(ec.KEPT_B)
    assert not (p[p[:, 5] == 1][:, 6] >= 0).any()
    toks = list(fixture['b_instances_token'])
    assert toks == ['inst0', 'inst1', 'inst6', 'inst0', 'inst1', 'inst2', 'inst6']      # inst2: a candidate in sweeps 0, 2, 3
    track_of = {tok: float(i) for i, tok in enumerate(dict.fromkeys(toks))}
    for k in (2, 3):
        raw = t['points'][k]
        keep = ec.kept_mask(raw[:, :2])
        rows = p[p[:, 5] == k]
        planted = rows[(np.cumsum(keep) - 1)[list(ec.PLANT_ROWS_B)], 6]
        assert (planted == track_of['inst1']).any() and (planted < 0).any()           # both sides of the truck's faces
        for row in (0, 63, 511, 512, 599):                                              # raw rows = lanes / tile rows
            assert keep[row]
        assert (rows[(np.cumsum(keep) - 1)[300:304], 6] == track_of['inst6']).all()    # inside car and bus: the bus wins
    assert (p[p[:, 5] == 3][:, 6] == track_of['inst2']).sum() == 1


@pytest.mark.parametrize('scenario', sorted(ec.SCENARIOS))
def test_device_contract_in_numpy_matches_reference(fixture, scenario, tmp_path):
    """collect_sweep_inputs + the kernel's contract (radius in un-fused f32, f64 FMA chains in k order through
    oracle.homo_transform, IEEE division, last box wins, tracks numbered by first hit in box order) = the fixture"""
    from datasets.nuscenes_sweeps import collect_sweep_inputs
    from oracle import oracle as orc
    c = ec.cfg(scenario)
    inputs = collect_sweep_inputs(fake(fixture, scenario, tmp_path), 'sample0', c['n_sweeps'], c['detection_classes'])
    points, tokens, centres = ec.contract_model(inputs, c['center_radius'], c['in_box_tolerance'], orc.homo_transform)
    want = ec.expected(fixture, scenario)
    assert np.array_equal(points, want['points'])
    assert tokens == list(want['instances_token'])
    assert np.array_equal(np.stack(centres), want['instances_center'])
