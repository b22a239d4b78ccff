"""Bit-identity evidence for a change to the estimators' training loop, on one GPU:

    python tools/estimator_bitwise.py --out new.npz          (in each of two checkouts)
    python tools/estimator_bitwise.py --compare old.npz new.npz --json bitwise.json

Fits a fixed list of small models with fixed seeds through the public API only (d = 1, n = 203,
batch 32, 4 epochs: six full batches and a partial one per epoch) and writes every trained tensor
and every ``history`` list to the ``.npz``; for the Bayesian models also one ``score`` and one
``evaluate(include_kl=True)``, which consume the posterior-draw generator.  ``--compare`` lists
every array with its shape and whether the two files hold the same bytes, and exits 1 if any
differs."""

import argparse
import itertools
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def cases():
    """``(tag, class name, constructor kwargs, fused_dense, fit kwargs)``."""
    out = []
    for graph, noise in itertools.product((True, False), (0.0, 0.1)):
        fit = dict(use_graph=graph)
        reg = dict(noise_reg=("fixed_rate", noise))
        tag = f"graph{int(graph)}_noise{noise}"
        for fused in (True, False):
            out.append((f"nfn_{tag}_fused{int(fused)}", "NormalizingFlowNetwork",
                        dict(n_flows=3, hidden_sizes=(16, 16), **reg), fused, fit))
        out.append((f"mdn_{tag}", "MixtureDensityNetwork", dict(n_centers=3, hidden_sizes=(4,), **reg), True, fit))
        out.append((f"kmn_{tag}", "KernelMixtureNetwork", dict(n_centers=5, hidden_sizes=(16, 16), **reg), True, fit))
        for variational in (True, False):
            vfit = dict(variational=variational, **fit)
            klw = dict(kl_weight_scale=1.0 / 203, **reg)
            out.append((f"bnfn_{tag}_variational{int(variational)}", "BayesNormalizingFlowNetwork",
                        dict(n_flows=2, hidden_sizes=(4,), **klw), True, vfit))
            if noise:
                out.append((f"bmdn_{tag}_variational{int(variational)}", "BayesMixtureDensityNetwork",
                            dict(n_centers=3, hidden_sizes=(16, 16), **klw), True, vfit))
                out.append((f"bkmn_{tag}_variational{int(variational)}", "BayesKernelMixtureNetwork",
                            dict(n_centers=5, hidden_sizes=(4,), **klw), True, vfit))
    vfit, klw = dict(variational=True, use_graph=True), dict(kl_weight_scale=1.0 / 203, hidden_sizes=(4,))
    out.append(("bnfn_map_mode", "BayesNormalizingFlowNetwork", dict(n_flows=2, map_mode=True, **klw), True, vfit))
    out.append(("bmdn_sampled_kl", "BayesMixtureDensityNetwork", dict(n_centers=3, kl_use_exact=False, **klw), True,
                vfit))
    out.append(("bkmn_trainable_prior", "BayesKernelMixtureNetwork",
                dict(n_centers=5, trainable_prior=True, prior_scale=0.5, **klw), True, vfit))
    return out


def run(out_path: str):
    import torch

    import normalizingflownetwork_amd as nfn

    assert torch.cuda.is_available(), "estimator_bitwise needs a HIP device"
    rng = np.random.default_rng(22)
    x = rng.uniform(-3, 3, (203, 1)).astype(np.float32)
    y = (np.cos(x) + 0.3 * rng.standard_normal((203, 1))).astype(np.float32)
    arrays = {}
    for i, (tag, cls, kwargs, fused, fit) in enumerate(cases()):
        m = getattr(nfn, cls)(1, **kwargs)
        m.fused_dense = fused
        hist = m.fit(x, y, batch_size=32, epochs=4, verbose=0, **fit)
        tensors = {f"w{k}": t for k, t in enumerate(m._mlp.weights)}
        tensors.update({f"b{k}": t for k, t in enumerate(m._mlp.biases)})
        for k, pair in enumerate(getattr(m, "_post_rho", None) or []):
            tensors[f"rho_w{k}"], tensors[f"rho_b{k}"] = pair
        if getattr(m, "_prior_loc", None) is not None:
            tensors["prior_loc"] = m._prior_loc
        if hasattr(m.dist_layer, "v"):
            tensors["v"] = m.dist_layer.v
        if hasattr(m.dist_layer, "locs"):
            tensors["locs"] = torch.as_tensor(np.asarray(m.dist_layer.locs))
        key = f"{i:02d}_{tag}"
        for name, t in tensors.items():
            arrays[f"{key}/{name}"] = t.detach().cpu().numpy()
        for name, values in hist.items():
            arrays[f"{key}/history_{name}"] = np.asarray(values, np.float64)
        if cls.startswith("Bayes"):
            arrays[f"{key}/score"] = np.asarray([m.score(x, y)], np.float64)
            arrays[f"{key}/evaluate_kl"] = np.asarray([m.evaluate(x, y, include_kl=True)], np.float64)
        print(f"{key}: loss {hist['loss']}", flush=True)
    np.savez(out_path, **arrays)
    print(f"wrote {len(arrays)} arrays of {len(cases())} models to {out_path}", flush=True)
    return 0


def compare(a_path: str, b_path: str, json_path: str):
    a, b = np.load(a_path), np.load(b_path)
    rows = []
    for name in sorted(set(a.files) | set(b.files)):
        if name not in a.files or name not in b.files:
            rows.append({"array": name, "shape": None, "equal": False})
            continue
        u, v = a[name], b[name]
        same = u.shape == v.shape and u.dtype == v.dtype and u.tobytes() == v.tobytes()
        rows.append({"array": name, "shape": list(u.shape), "dtype": str(u.dtype), "equal": bool(same)})
    result = {"tool": "estimator_bitwise", "arrays": len(rows), "all_equal": all(r["equal"] for r in rows),
              "differing": [r["array"] for r in rows if not r["equal"]], "rows": rows}
    with open(json_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("tool", "arrays", "all_equal", "differing")}), flush=True)
    return 0 if result["all_equal"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("OLD", "NEW"))
    ap.add_argument("--json", default="bitwise.json")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare, args.json)
    assert args.out, "give --out FILE.npz or --compare OLD NEW"
    return run(args.out)


if __name__ == "__main__":
    sys.exit(main())
