"""Mesh -> down-sampled point set + nearest-vertex index map, in the pickle schema the ComA stage reads.

Mirrors the two writers of the reference, `src/coma/downsample_human.py:17-77` and `src/coma/downsample_objects.py:17-60`
(keys, dtypes and the two zero-normal filters), with the open3d pieces replaced:
  * nearest vertex  -> coma_nearest_vertex_i64 (bit-exact argmin, utils/coma.py:87-91);
  * vertex normals  -> coma_vertex_normals_f64 (area-weighted, ascending-face accumulation like open3d; parity unpinned --
    open3d is absent from the build image);
  * the point sampler: open3d's own Poisson-disk point set is third party and is never silently replaced;
    for simplify_method="poisson_disk" points are SUPPLIED (what a maintainer with open3d exports once; sampler="supplied", the
    default, which raises without them) or, only when the caller opts in with sampler="device", drawn by sample_poisson_disk
    below; simplify_method="uniform" draws with the seeded area-weighted uniform sampler.

sample_poisson_disk is weighted sample elimination (Yuksel 2015), the method behind open3d's sample_points_poisson_disk, run by
coma_sample_eliminate_f64 bit-identically to its NumPy restatement (tests/sample_elim_ref.py).  Parity with open3d's own point set
is UNPINNED: open3d draws its candidates with another RNG, and the constants below are quoted from memory of its source.  What is
pinned is the algorithm as include/coma_hip.h states it.
"""
from __future__ import annotations

import numpy as np

import torch

from . import _lib
from .coma import nearest_vertex_indices
from .ingest import vertex_normals_batch


def load_obj(pth):
    """Vertices and triangles of a Wavefront OBJ in file order (faces fan-triangulated, v/vt/vn index forms accepted)."""
    verts, faces = [], []
    with open(pth) as fh:
        for line in fh:
            t = line.split()
            if not t:
                continue
            if t[0] == "v":
                verts.append([float(x) for x in t[1:4]])
            elif t[0] == "f":
                idx = [int(tok.split("/")[0]) for tok in t[1:]]
                idx = [i - 1 if i > 0 else len(verts) + i for i in idx]
                faces += [[idx[0], idx[k], idx[k + 1]] for k in range(1, len(idx) - 1)]
    return np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int64)


def sample_uniform(vertices, faces, vertex_normals, number_of_points, seed=0):
    """Seeded area-weighted uniform surface samples with barycentric-interpolated, re-normalised normals."""
    rng = np.random.default_rng(seed)
    a, b, c = (vertices[faces[:, k]] for k in range(3))
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    f = rng.choice(len(faces), size=number_of_points, p=area / area.sum())
    r1, r2 = np.sqrt(rng.random(number_of_points)), rng.random(number_of_points)
    w = np.stack([1 - r1, r1 * (1 - r2), r1 * r2], axis=1)
    pts = (w[:, :, None] * vertices[faces[f]]).sum(1)
    nrm = (w[:, :, None] * vertex_normals[faces[f]]).sum(1)
    n = np.linalg.norm(nrm, axis=1, keepdims=True)
    return pts, np.divide(nrm, n, out=np.zeros_like(nrm), where=n > 0)


# [3rd-party, from memory of open3d's source, unpinned]: the constants of TriangleMesh::SamplePointsPoissonDisk.  They are
# arguments all the way down to the kernel, so a maintainer with open3d at hand can correct them here without touching it.
POISSON_INIT_FACTOR = 5      # candidates drawn per requested point
POISSON_ALPHA = 8.0          # weight exponent (the kernel refuses any other value: ((t*t)^2)^2 needs no pow)
POISSON_BETA = 0.5           # r_min = r_max * beta * (1 - (N/M)^gamma)
POISSON_GAMMA = 1.5


def poisson_radii(area, number_of_points, number_of_candidates, beta=POISSON_BETA, gamma=POISSON_GAMMA):
    """(r_max, r_min) of the elimination for N points kept out of M candidates on a surface of area A, in f64."""
    n, m = float(number_of_points), float(number_of_candidates)
    r_max = 2.0 * float(np.sqrt((float(area) / n) / (2.0 * np.sqrt(3.0))))
    return r_max, r_max * beta * (1.0 - (n / m) ** gamma)


def sample_eliminate(points, n_keep, r_max, r_min, alpha=POISSON_ALPHA, device="cuda"):
    """coma_sample_eliminate_f64: indices (ascending, i64 [n_keep]) of the candidates that survive weighted sample elimination."""
    L = _lib.lib()
    pts = torch.tensor(np.ascontiguousarray(np.asarray(points, dtype=np.float64)), device=device)
    assert pts.dim() == 2 and pts.shape[1] == 3
    M = pts.shape[0]
    ws = torch.empty([max(1, int(L.coma_sample_eliminate_workspace_bytes(M)) // 8)], dtype=torch.float64, device=pts.device)
    keep = torch.empty([max(0, int(n_keep))], dtype=torch.int64, device=pts.device)
    rc = L.coma_sample_eliminate_f64(_lib.ptr(pts, torch.float64), M, int(n_keep), float(r_max), float(r_min), float(alpha),
                                     _lib.ptr(ws), _lib.ptr(keep, torch.int64), _lib.stream_ptr(pts.device))
    _lib.check(rc, "coma_sample_eliminate_f64")
    return keep.cpu().numpy()


def sample_poisson_disk(vertices, faces, vertex_normals, number_of_points, seed=0, device="cuda", init_factor=POISSON_INIT_FACTOR):
    """Blue-noise surface samples: init_factor * N seeded uniform candidates (sample_uniform, same seed semantics) thinned to N by
    weighted sample elimination on the device.  Returns the kept points and their normals in ascending candidate order.
    NOT open3d's point set (see the module docstring): same method, another RNG, constants unpinned."""
    n = int(number_of_points)
    m = int(init_factor) * n
    pts, nrm = sample_uniform(vertices, faces, vertex_normals, m, seed)
    a, b, c = (np.asarray(vertices, dtype=np.float64)[faces[:, k]] for k in range(3))
    area = float((0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)).sum())
    r_max, r_min = poisson_radii(area, n, m)
    keep = sample_eliminate(pts, n, r_max, r_min, POISSON_ALPHA, device=device)
    return pts[keep], nrm[keep]


SAMPLERS = ("supplied", "device")


def _points(vertices, faces, normals, number_of_points, points, point_normals, simplify_method, seed, sampler="supplied", device="cuda"):
    assert sampler in SAMPLERS, f"sampler: '{sampler}' not in {SAMPLERS}"
    if points is not None:
        points = np.asarray(points, dtype=np.float64)
        assert point_normals is not None and len(point_normals) == len(points), "supplied points need their normals"
        return points, np.asarray(point_normals, dtype=np.float64)
    if simplify_method != "uniform":
        if sampler == "device":
            return sample_poisson_disk(vertices, faces, normals, number_of_points, seed, device)
        raise NotImplementedError("Poisson-disk sampling is open3d's (third party): pass points=/point_normals= exported from it, "
                                  "opt in to the device sampler with sampler='device' (same method, not open3d's point set), "
                                  "or use simplify_method='uniform'")
    return sample_uniform(vertices, faces, normals, number_of_points, seed)


def downsample_human(vertices, faces, number_of_points, points=None, point_normals=None, simplify_method="uniform", seed=42, device="cuda",
                     sampler="supplied"):
    """downsample_human.py:29-77 -> the dict it pickles as smplx_star_downsampled_{N}.pickle."""
    vertices, faces = np.asarray(vertices), np.asarray(faces).astype(np.int64)
    V = len(vertices)
    normals = vertex_normals_batch(vertices, faces, device=device)[0]
    if number_of_points < V:
        pts, nrm = _points(vertices.astype(np.float64), faces, normals, number_of_points, points, point_normals, simplify_method, seed,
                           sampler, device)
        indices = [int(i) for i in nearest_vertex_indices(pts, vertices.astype(np.float64), device=device)]
    else:
        pts, nrm, indices = vertices.astype(np.float64), normals, list(range(V))
    indices = [i for i in indices if normals[i].sum() != 0]          # vertices without a normal are skipped (:58-65)
    return {"vertices": vertices, "faces": faces, "V": V, "F": faces.shape[0], "N": len(indices), "N_raw": len(pts),
            "downsample_indices": indices, "downsampled_pcd_points_raw": pts, "downsampled_pcd_normal_raw": nrm}


def downsample_object(supercategory, category, asset_id, vertices, faces, number_of_points, points=None, point_normals=None,
                      simplify_method="uniform", seed=42, device="cuda", sampler="supplied"):
    """downsample_objects.py:17-62 -> the dict it pickles as {asset_id}_{N}.pickle."""
    vertices, faces = np.asarray(vertices, dtype=np.float64), np.asarray(faces).astype(np.int64)
    normals = vertex_normals_batch(vertices, faces, device=device)[0]
    pts, nrm = _points(vertices, faces, normals, number_of_points, points, point_normals, simplify_method, seed, sampler, device)
    indices = [int(i) for i in nearest_vertex_indices(pts, vertices, device=device)]
    keep = np.array([d for d in range(len(nrm)) if nrm[d].sum() != 0], dtype=np.int64)   # zero-normal samples are dropped (:30-38)
    return {"supercategory": supercategory, "category": category, "asset_id": asset_id, "V": vertices.shape[0], "F": faces.shape[0],
            "N": len(indices), "N_raw": len(keep), "downsample_indices": indices, "downsampled_pcd_points_raw": pts[keep],
            "downsampled_pcd_normal_raw": nrm[keep], "obj_vertices_original": vertices, "obj_faces_original": faces,
            "obj_vertex_normals_original": normals}
