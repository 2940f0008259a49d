"""Meshes and file fixtures shared by tests/test_metrics_host.py and tests/test_metrics_gpu.py."""
import os
import pickle

import numpy as np

from tests import raster_ref as RR


def rot(axis, angle):
    """Rodrigues rotation matrix."""
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def flipped(mesh):
    return mesh[0], np.ascontiguousarray(mesh[1][:, ::-1])


def convex_pairs():
    """The three convex pairs whose exact intersection volume SciPy can give."""
    c1 = RR.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    c2 = RR.box((-0.45, -0.55, -0.4), (0.55, 0.45, 0.6))
    a = (c1[0] @ rot((1, 2, 3), 0.7).T, c1[1])
    b = (c2[0] @ rot((-2, 1, 0.5), 1.1).T + np.array([0.21, -0.13, 0.17]), c2[1])
    tet = (np.array([[0.9, 0.1, -0.6], [-0.7, 0.8, -0.5], [-0.6, -0.9, -0.4], [0.05, 0.1, 0.95]]),
           np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=np.int32))
    return dict(cubes=(a, b), cube_tet=(a, tet), spheres=(RR.icosphere(2, 0.8), RR.icosphere(2, 0.7, (0.45, 0.3, -0.25))))


def grazing_pair():
    """A sphere and a box whose bounding boxes overlap by 5 mm x 3 mm at a corner: cells of 1/512 of that overlap would put the far
    vertices beyond the device's coordinate range, so the grid's scale must be capped."""
    return RR.icosphere(3, 0.9), RR.box((0.895, 0.897, -0.2), (1.5, 1.4, 0.3))


def grazing_boxes():
    """Two boxes that share 4 mm x 3 mm x 0.6 at a corner (exact intersection volume 7.2e-6): the same cap, with a volume to find."""
    return RR.box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), RR.box((0.996, 0.997, 0.2), (2.0, 2.0, 0.8))


def slab_stack(n, lo, hi, z0, pitch, thickness):
    """n thin boxes over the same xy rectangle, one mesh."""
    vs, fs = [], []
    for k in range(n):
        v, f = RR.box((lo[0], lo[1], z0 + k * pitch), (hi[0], hi[1], z0 + k * pitch + thickness))
        fs.append(f + 8 * k), vs.append(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def write_obj(pth, verts, faces):
    """Wavefront OBJ with round-tripping coordinates (repr of a float parses back to the same float)."""
    os.makedirs(os.path.dirname(pth), exist_ok=True)
    with open(pth, "w") as fh:
        for v in np.asarray(verts, dtype=np.float64).tolist():
            fh.write(f"v {v[0]!r} {v[1]!r} {v[2]!r}\n")
        for f in np.asarray(faces).tolist():
            fh.write(f"f {f[0] + 1} {f[1] + 1} {f[2] + 1}\n")


def write_pickle(pth, payload):
    os.makedirs(os.path.dirname(pth), exist_ok=True)
    with open(pth, "wb") as fh:
        pickle.dump(payload, fh)


def relative_files(root, ext):
    out = []
    for d, _, files in os.walk(root):
        out += [os.path.relpath(os.path.join(d, f), root) for f in files if f.endswith(ext)]
    return sorted(out)
