"""One call each of the entry points that scan or sort, at fixed seeded sizes: the kernel-trace summary of this script
counts their dispatches."""
import sys

import numpy as np

sys.path.insert(0, ".")
from multimesh_amd import synth
from multimesh_amd.device import Context

ctx = Context(0)
rng = np.random.default_rng(0)
pa, ca = synth.hex_mesh(65, seed=1)                      # 64^3 elements
corners = ctx.to_device(pa[ca].reshape(-1, 3))           # 2.1 M rows, each node up to 8 times
for _ in range(2):
    uniq, inv = ctx.unique_points(corners)
    uniq2, inv2 = ctx.unique_points(corners, ordered=False)
    faces, nonmanifold = ctx.boundary_faces(inv2.reshape(len(ca), 8), uniq2.shape[0])
    # structured rows: the general path of the ordered unique
    g = np.stack(np.meshgrid(*[np.arange(40.0)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    ctx.unique_points(ctx.to_device(np.concatenate([g, g[::3]])))
    # transpose create: 8 contributions per target onto 200 k destinations
    n, nsrc = 500_000, 200_000
    ids = ctx.to_device(rng.integers(0, nsrc, size=(n, 8)))
    w = ctx.to_device(rng.uniform(size=(n, 8)))
    op = ctx.transpose_nodes(ids, w, nsrc)
    op.free()
    # a graded cloud: the kNN tree's sort
    src, tgt = rng.uniform(size=(400_000, 3)) ** 3.0, rng.uniform(size=(400_000, 3)) ** 3.0
    tree = ctx.knn_build(ctx.to_device(src))
    tree.query(ctx.to_device(tgt), 20)
    kernels = sorted(ctx.last_knn_kernels())
    # a uniform cloud: grid build with the statistic, target sort, lane work list
    src, tgt = rng.uniform(size=(400_000, 3)), rng.uniform(size=(400_000, 3))
    ctx.knn_build(ctx.to_device(src)).query(ctx.to_device(tgt), 8)
    kernels2 = sorted(ctx.last_knn_kernels())
ctx.synchronize()
print("unique", uniq.shape[0], uniq2.shape[0], "faces", faces.shape[0], "knn", kernels, kernels2)
