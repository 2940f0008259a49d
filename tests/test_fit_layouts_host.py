"""The buffer sizes of the fitting modules, pinned as literals (no GPU).

The `*_workspace_bytes`, `*_saved_bytes` and `*_state_bytes` functions are the visible end of the Layout builders of
csrc/smplx.hip, vposer.hip, app_objective.hip and of mesh_volume.hip's partials: a `saved` buffer written by one build's forward is
read by another build's backward only while every offset stays where it is.  The numbers were read off the library BEFORE the
builders moved to the shared carving helper of csrc/common.h; each set holds the app's own sizes, odd counts that exercise the
rounding to 16 bytes, the limits of the accepted domain, and refused tuples (0).
"""
import pytest

PINNED = {
    "coma_smplx_workspace_bytes": {(10475, 55): 2705312, (7, 5): 2608, (129, 64): 49296, (1, 1): 384, (1 << 24, 64): 4432339840,
                                   (0, 5): 0, (7, 65): 0, ((1 << 24) + 1, 5): 0},
    "coma_smplx_shape_state_bytes": {(10475, 55): 252736, (7, 5): 304, (129, 64): 4640, (1, 1): 64, (0, 5): 0, (7, 65): 0},
    "coma_smplx_saved_bytes": {(10475, 55): 258016, (7, 5): 784, (129, 64): 10784, (1, 1): 160, (0, 5): 0, (7, 65): 0},
    "coma_vposer_saved_bytes": {(1, 512, 21): 9232, (3, 33, 1): 1760, (64, 2048, 64): 2297856, (2, 7, 5): 720, (0, 512, 21): 0,
                                (65, 512, 21): 0, (1, 2049, 21): 0, (1, 512, 65): 0},
    "coma_vposer_workspace_bytes": {(1, 512, 21): 12288, (3, 33, 1): 2400, (64, 2048, 64): 3145728, (2, 7, 5): 1440, (0, 512, 21): 0,
                                    (65, 512, 21): 0, (1, 2049, 21): 0, (1, 512, 65): 0},
    # (V, F, k): k = 0 drops the contact term's arrays to their 16-byte minimum, k = 65 is one row past a 64-row tile
    "coma_app_objective_workspace_bytes": {(10475, 20908, 0): 251744, (10475, 20908, 1): 251824, (10475, 20908, 1000): 531808,
                                           (10475, 20908, 10475): 1509408, (7, 5, 0): 192, (7, 5, 1): 272, (7, 5, 7): 512,
                                           (300, 596, 65): 10880, (7, 5, 8): 0, (0, 5, 0): 0, (7, 0, 0): 0, (7, 5, -1): 0},
    # one f64 per workgroup of 256 faces, 256 workgroups at the most
    "coma_mesh_volume_workspace_bytes": {(1,): 8, (255,): 8, (256,): 8, (257,): 16, (20908,): 656, (65536,): 2048, (65537,): 2048,
                                         (1000000,): 2048, (0,): 0, (-3,): 0},
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_buffer_sizes_are_where_they_were(hip_lib, name):
    fn = getattr(hip_lib, name)
    got = {args: int(fn(*args)) for args in PINNED[name]}
    assert got == PINNED[name]
