#!/usr/bin/env python3
"""Generate tests/golden/rotation.npz: the reference's own ``get_rot_matrix`` and ``rotate`` on seeded inputs.

Run in a container that has the reference checkout:   python tests/golden/make_rotation_golden.py [REFERENCE_ROOT]
(default /root/reference).

The reference's multi_mesh/utils.py cannot be imported without geographiclib, pyexodus, h5py, xarray and salvus, none of
which these two functions use.  They are taken from that file at run time -- parsed with ``ast``, their definitions alone
executed in a namespace holding ``np`` -- so the expected outputs are the reference's statements evaluated by NumPy.

Arrays only; no reference source text:
* ``angles`` f64[M] in DEGREES and ``axes`` f64[M, 3]: the reference is handed ``np.deg2rad(angle)`` and the axis's three
  components as NumPy scalars.  They include the angles 0 and 180 and axes that are not normalised.
* ``matrices`` f64[M, 3, 3]: what ``get_rot_matrix`` returned.
* ``points`` f64[M, K, 3] at Earth scale and ``rotated`` f64[M, K, 3]: ``rotate`` of block m by matrix m (its [3, K] result
  transposed).
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
M, K = 20, 50


def reference_functions(reference_root, names=("get_rot_matrix", "rotate")):
    path = os.path.join(reference_root, "multi_mesh", "utils.py")
    tree = ast.parse(open(path).read(), filename=path)
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in nodes) == sorted(names)
    namespace = {"np": np}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), namespace)
    return [namespace[n] for n in names]


def main():
    reference_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    get_rot_matrix, rotate = reference_functions(reference_root)
    rng = np.random.default_rng(20261021)

    angles = rng.uniform(-360.0, 360.0, M)
    angles[:4] = [0.0, 180.0, 90.0, -1e-7]
    axes = rng.normal(size=(M, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    axes[4:10] *= rng.uniform(1e-3, 1e7, (6, 1))            # not normalised
    axes[10:13] = [[0.0, 0.0, 1.0], [0.0, -2.0, 0.0], [3.0, 0.0, 0.0]]
    axes[1] = [1.0, 2.0, -3.0]                              # the half turn, about an axis that is not normalised
    d = rng.normal(size=(M, K, 3))
    points = d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(3.4e6, 6.371e6, (M, K, 1))

    matrices = np.empty((M, 3, 3))
    rotated = np.empty((M, K, 3))
    for m in range(M):
        x, y, z = (np.float64(a) for a in axes[m])
        matrices[m] = get_rot_matrix(np.deg2rad(angles[m]), x, y, z)
        rotated[m] = rotate(points[m, :, 0], points[m, :, 1], points[m, :, 2], matrices[m]).T
    assert np.array_equal(matrices[0], np.eye(3)) and np.isfinite(matrices).all() and not np.array_equal(rotated[1], points[1])

    np.savez_compressed(os.path.join(HERE, "rotation.npz"), angles=angles, axes=axes, matrices=matrices, points=points,
                        rotated=rotated)
    print("wrote", os.path.join(HERE, "rotation.npz"))


if __name__ == "__main__":
    main()
