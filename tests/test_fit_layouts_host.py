"""The buffer sizes of the fitting modules, pinned as literals (no GPU).

The `*_workspace_bytes`, `*_saved_bytes` and `*_state_bytes` functions are the visible end of the Layout builders of
csrc/smplx.hip, vposer.hip, app_objective.hip and of mesh_volume.hip's partials: a `saved` buffer written by one build's forward is
read by another build's backward only while every offset stays where it is.  The numbers were read off the library BEFORE the
builders moved to the shared carving helper of csrc/common.h; each set holds the app's own sizes, odd counts that exercise the
rounding to 16 bytes, the limits of the accepted domain, and refused tuples (0).
"""
import pytest

PINNED = {
    "coma_smplx_workspace_bytes": {(10475, 55): 2705312, (129, 5): 29456, (300, 55): 88496, (7, 5): 2608, (129, 64): 49296, (1, 1): 384,
                                   (1 << 24, 64): 4432339840, (0, 5): 0, (7, 65): 0, ((1 << 24) + 1, 5): 0},
    "coma_smplx_shape_state_bytes": {(10475, 55): 252736, (129, 5): 3232, (300, 55): 8528, (7, 5): 304, (129, 64): 4640, (1, 1): 64,
                                     (0, 5): 0, (7, 65): 0},
    "coma_smplx_saved_bytes": {(10475, 55): 258016, (129, 5): 3712, (300, 55): 13808, (7, 5): 784, (129, 64): 10784, (1, 1): 160,
                               (0, 5): 0, (7, 65): 0},
    # (V, J, NB) and (V, J, N), read off the library BEFORE the single-body and batched layouts of csrc/smplx.hip became one builder
    "coma_smplx_grad_workspace_bytes": {(129, 5, 0): 7648, (129, 5, 20): 7952, (300, 55, 0): 35568, (300, 55, 20): 36176,
                                        (10475, 55, 0): 943952, (10475, 55, 20): 962640, (0, 5, 0): 0, (129, 5, -1): 0, (129, 5, 1025): 0},
    "coma_smplx_batch_workspace_bytes": {(129, 5, 1): 25056, (129, 5, 2): 50112, (129, 5, 8): 200448, (129, 5, 9): 225504,
                                         (129, 5, 1024): 25657344, (300, 55, 1): 61488, (300, 55, 2): 122976, (300, 55, 8): 491904,
                                         (300, 55, 9): 553392, (300, 55, 1024): 62963712, (10475, 55, 1): 2015088, (10475, 55, 2): 4030176,
                                         (10475, 55, 8): 16120704, (10475, 55, 9): 18135792, (10475, 55, 1024): 2063450112,
                                         (129, 5, 0): 0, (129, 5, 1025): 0, (0, 5, 2): 0},
    "coma_smplx_batch_saved_bytes": {(129, 5, 1): 3712, (129, 5, 2): 7424, (129, 5, 8): 29696, (129, 5, 9): 33408, (129, 5, 1024): 3801088,
                                     (300, 55, 1): 13808, (300, 55, 2): 27616, (300, 55, 8): 110464, (300, 55, 9): 124272,
                                     (300, 55, 1024): 14139392, (10475, 55, 1): 258016, (10475, 55, 2): 516032, (10475, 55, 8): 2064128,
                                     (10475, 55, 9): 2322144, (10475, 55, 1024): 264208384, (129, 5, 0): 0, (129, 5, 1025): 0, (0, 5, 2): 0},
    "coma_smplx_batch_grad_workspace_bytes": {(129, 5, 1): 7504, (129, 5, 2): 14976, (129, 5, 8): 59904, (129, 5, 9): 67408,
                                              (129, 5, 1024): 7667712, (300, 55, 1): 34208, (300, 55, 2): 68400, (300, 55, 8): 273600,
                                              (300, 55, 9): 307808, (300, 55, 1024): 35020800, (10475, 55, 1): 941632, (10475, 55, 2): 1883232,
                                              (10475, 55, 8): 7532928, (10475, 55, 9): 8474560, (10475, 55, 1024): 964214784,
                                              (129, 5, 0): 0, (129, 5, 1025): 0, (0, 5, 2): 0},
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
