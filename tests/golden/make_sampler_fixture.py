"""Writes tests/golden/sampler_flows.npz: the flow parameters of tests/test_sampler_backward_{cpu,gpu}.py.

Only oracle/ is used; it runs in seconds on the CPU:  python tests/golden/make_sampler_fixture.py

Stored: parameter blobs (torch layout, float32), the two training batches and the seeds.  Every blob is trained-like:
  * `O.init_blob` + 0.25 * randn per layer (the `make_problem` recipe of tests/test_hip_parity.py), one per row of RECIPES;
  * two flows trained by `CO.train` (float32, lr 0.02, window 50, tolerance 1e-2) on a banana-plus-bimodal batch standardised
    per column: (n = 1000, D = 3, K = 5, H = 8, at most 600 iterations) and (n = 600, D = 4, K = 9, H = 8, at most 300).
No noise amplitude above 0.5 is used anywhere; the latent draws and normalisation constants are made by the tests from seeds.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import c_oracle as CO          # noqa: E402
from oracle import nsf_torch as O          # noqa: E402

# name -> (model_D, K, H, L, seed)
RECIPES = {
    "d1": (1, 9, 8, 1, 101), "d5": (5, 9, 8, 1, 102), "d12": (12, 9, 8, 1, 103), "d5k2": (5, 2, 8, 1, 104),
    "d5k16": (5, 16, 8, 1, 105), "d20h16": (20, 9, 16, 1, 106), "d12k5h4": (12, 5, 4, 1, 107), "d5l2": (5, 9, 8, 2, 108),
    "d7l2": (7, 9, 8, 2, 109), "d7l3": (7, 9, 8, 3, 110), "d12h16l2": (12, 9, 16, 2, 111),
    "d9l2": (9, 9, 8, 2, 112),                                   # evaluated as its 6-dim marginal (layer stride)
}
# the three cliques of the walk tree (model dims 5, 8, 7) per (L, H), and the single-clique trees around the LDS switch
for L, H in ((1, 8), (1, 16), (1, 4), (2, 8)):
    for c, D in enumerate((5, 8, 7)):
        RECIPES["walk_l%dh%d_c%d" % (L, H, c)] = (D, 9, H, L, 200 + 10 * (4 * L + H) + c)
RECIPES["walk_d19h16"] = (19, 9, 16, 1, 301)
RECIPES["walk_d20h16"] = (20, 9, 16, 1, 302)


def recipe_blob(D, K, H, L, seed):
    gen = torch.Generator().manual_seed(seed)
    blob = torch.cat([O.init_blob(D, K, H, gen) for _ in range(L)])
    blob = blob + 0.25 * torch.randn(blob.shape, generator=gen)
    return blob.numpy().astype(np.float32)


def banana_bimodal(n, D, seed):
    rng = np.random.RandomState(seed)
    x = rng.randn(n, D)
    x[:, 1] = x[:, 0] ** 2 + 0.5 * rng.randn(n)                                  # banana
    x[:, 2] = np.where(rng.rand(n) < 0.4, -2.0, 2.0) + 0.5 * rng.randn(n)         # two modes
    x = (x - x.mean(0)) / x.std(0)
    return x.astype(np.float32)


def main():
    out = {}
    names = sorted(RECIPES)
    out["recipe_names"] = np.array(names)
    out["recipe_shapes"] = np.array([RECIPES[k] for k in names], dtype=np.int32)
    for k in names:
        out["blob_" + k] = recipe_blob(*RECIPES[k])
    for name, (n, D, K, H, iters, seed) in {"trained3": (1000, 3, 5, 8, 600, 401), "trained4": (600, 4, 9, 8, 300, 402)}.items():
        x = banana_bimodal(n, D, seed)
        gen = torch.Generator().manual_seed(seed)
        b0 = O.init_blob(D, K, H, gen).numpy()
        blob, loss, it, _, _ = CO.train(x, b0, K, H, 5.0, 1, lr=0.02, max_iters=iters, average_window=50, loss_delta_tol=1e-2,
                                        early_stop=True, dtype=np.float32)
        print("%s: stopped after %d iterations, loss %.4f -> %.4f" % (name, it, loss[0], loss[it - 1]))
        out["blob_" + name] = blob.astype(np.float32)
        out["x_" + name] = x
        out["shape_" + name] = np.array([D, K, H, 1, seed, it], dtype=np.int32)
    path = os.path.join(HERE, "sampler_flows.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
