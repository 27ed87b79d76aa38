"""Every exported function of include/pca.h that takes a pca_ctx has its refusals tested, and this says where (no GPU needed).

Each such function is in exactly one of
  core_refusals_common.TABLES   its refused calls, run by tests/test_gpu_core_refusals.py;
  COVERED_ELSEWHERE             symbol -> 'tests/file.py::test_name': that file defines that test and names the symbol or its
                                wrapper (WRAPPERS);
  EXEMPT                        symbol -> reason; never an entry point that launches a kernel.
A new entry point fails this test until it is put into one of them."""
import os
import re

import core_refusals_common as cr
from conftest import ROOT

REFUSALS = 'test_refusals_launch_nothing_and_leave_the_outputs_alone'
COVERED_ELSEWHERE = {
    'pca_nusc_merge_sweeps': 'tests/test_gpu_nusc_sweeps.py::test_device_merger_limits',
    'pca_bev_class_planes': 'tests/test_gpu_sem_planes.py::test_edges_and_refusals',
    'pca_bev_elev_partition': 'tests/test_gpu_elev_partition.py::test_refusals_the_cut_window_and_empty_windows',
    'pca_bev_voxel_labels': 'tests/test_gpu_voxel_labels.py::' + REFUSALS,
    'pca_bev_voxel_rays': 'tests/test_gpu_voxel_rays.py::' + REFUSALS,
    'pca_bev_voxel_carve': 'tests/test_gpu_voxel_carve.py::' + REFUSALS,
    'pca_bev_voxel_instances': 'tests/test_gpu_voxel_instances.py::' + REFUSALS,
    'pca_bev_instance_boxes': 'tests/test_gpu_instance_boxes.py::' + REFUSALS,
    'pca_render_camera': 'tests/test_gpu_render_camera.py::' + REFUSALS,
    'pca_bev_voxel_camera': 'tests/test_gpu_voxel_camera.py::' + REFUSALS,
    'pca_voxel_pool': 'tests/test_gpu_voxel_ssc.py::' + REFUSALS,
    'pca_voxel_pack': 'tests/test_gpu_voxel_ssc.py::' + REFUSALS,
    'pca_voxel_distance': 'tests/test_gpu_voxel_distance.py::' + REFUSALS,
    'pca_voxel_instance_match': 'tests/test_gpu_voxel_tracks.py::test_refused_calls_write_nothing',
    'pca_lanes_transform': 'tests/test_gpu_lanes.py::test_bad_arguments_are_refused',
    'pca_lanes_to_grid': 'tests/test_gpu_lanes.py::test_bad_arguments_are_refused',
}
WRAPPERS = {                 # what a test file says instead of the symbol: the binding it calls
    'pca_bev_class_planes': 'bev_class_planes', 'pca_bev_elev_partition': 'bev_elev_partition', 'pca_bev_voxel_labels': 'bev_voxel_labels',
    'pca_bev_voxel_rays': 'bev_voxel_rays', 'pca_bev_voxel_carve': 'bev_voxel_carve', 'pca_bev_voxel_instances': 'bev_voxel_instances',
    'pca_bev_instance_boxes': 'bev_instance_boxes', 'pca_render_camera': 'render_camera', 'pca_bev_voxel_camera': 'bev_voxel_camera',
    'pca_voxel_pool': 'voxel_pool', 'pca_voxel_pack': 'voxel_pack', 'pca_voxel_distance': 'voxel_distance',
    'pca_voxel_instance_match': 'voxel_instance_match', 'pca_lanes_transform': 'lanes_transform', 'pca_lanes_to_grid': 'lanes_to_grid',
    'pca_nusc_merge_sweeps': 'merge_sweeps',
}
EXEMPT = {
    'pca_ctx_destroy': 'returns nothing; frees the context and launches nothing (a noted K1 is dropped, not run)',
    'pca_last_error': 'a read of the context\'s message; "null context" without one',
    'pca_status_peek': 'a read of mapped host words; no stream operation',
    'pca_status_mirror': 'returns an address',
    'pca_profile_enable': 'the profiler\'s switch: synchronises recorded events, launches nothing',
    'pca_profile_read': 'the profiler\'s counters: synchronises recorded events, launches nothing',
    'pca_debug_bev_level1': 'a diagnostic: copies four ints of the context',
}
LAUNCHES = re.compile(r'hipLaunchKernelGGL|PCA_LAUNCH|pca_k1_flush_pending|pca_fetch_block')


def ctx_functions():
    """The functions of include/pca.h whose first parameter is a pca_ctx pointer (tests/test_abi.py reads the header the same way)."""
    text = open(os.path.join(ROOT, 'include', 'pca.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(pca_[a-z0-9_]+)\s*\(\s*(?:const\s+)?pca_ctx\s*\*\s*ctx\b', text)))


def body_of(symbol):
    """The definition of an exported function in csrc/, from its name to the closing brace in column 0."""
    src = os.path.join(ROOT, 'pc-accumulation-lib_amd', 'csrc')
    for f in sorted(os.listdir(src)):
        if f.endswith('.hip'):
            text = open(os.path.join(src, f)).read()
            hit = re.search(r'^[^\n;]*\b%s\s*\([^;{]*\)\s*\{' % symbol, text, flags=re.M)
            if hit:
                line_end = text.find('\n', hit.end())
                one_line = '}' in text[hit.end():line_end]
                return text[hit.start():line_end if one_line else text.index('\n}', hit.end())]
    raise AssertionError('no definition of %s under csrc/' % symbol)


def test_the_header_has_the_functions_this_is_about():
    names = ctx_functions()
    assert len(names) >= 50 and 'pca_bev_generate_chain' in names and 'pca_ctx_create' not in names and 'pca_host_view_hull' not in names


def test_every_ctx_entry_point_is_in_exactly_one_place():
    places = {'TABLES': set(cr.TABLES), 'COVERED_ELSEWHERE': set(COVERED_ELSEWHERE), 'EXEMPT': set(EXEMPT)}
    for name in ctx_functions():
        where = [k for k, v in places.items() if name in v]
        assert len(where) == 1, (name, where)
    listed = set().union(*places.values())
    assert listed == set(ctx_functions()), sorted(listed ^ set(ctx_functions()))


def test_every_table_has_cases_with_a_message():
    for symbol, table in cr.TABLES.items():
        assert len(table) >= 1, symbol
        labels = [label for label, _, _ in table]
        assert len(set(labels)) == len(labels), symbol
        for label, bad, msg in table:
            assert isinstance(bad, dict) and bad and re.compile(msg), (symbol, label)


def test_covered_elsewhere_names_tests_that_exist_and_speak_of_the_symbol():
    for symbol, where in COVERED_ELSEWHERE.items():
        path, test = where.split('::')
        text = open(os.path.join(ROOT, path)).read()
        assert re.search(r'^def %s\(' % re.escape(test), text, flags=re.M), where
        assert re.search(r'\b%s\b' % symbol, text) or re.search(r'\b%s\b' % WRAPPERS[symbol], text), (symbol, where)


def test_nothing_exempt_launches_a_kernel():
    for symbol, reason in EXEMPT.items():
        assert reason and not LAUNCHES.search(body_of(symbol)), symbol
    assert LAUNCHES.search(body_of('pca_bev_warp')) and LAUNCHES.search(body_of('pca_status'))       # (the search finds launches)
