"""Worst relative error of K5's log P(X > k) against tests/golden/poisson_edge_vectors.json, per family of the file and, in the
`outer` family (max(k, lambda) above 8192), per size -- the figures DESIGN section 5 quotes.  The error of a row is
|got - want| / max(1, |want|) over the rows whose p is a normal double, as tests/test_gpu_poisson.py asserts it.

    python tools/poisson_error_profile.py --out profiles/r11_poisson_error.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (10000, 16384, 32768, 100000, 300000, 1 << 20)  # k of the `outer` rows with lambda / k = 0.9 ... 1.1
sys.path.insert(0, ROOT)


def worst(rows):
    if not rows:
        return None
    r = max(rows, key=lambda r: r["err"])
    return {"rows": len(rows), "worst_relative_error": r["err"], "at": {"lambda": r["lam"], "k": r["k"], "logp": float(r["logp"]), "got": r["got"]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    from breakdancer_amd.api import poisson_log_upper_tail
    v = json.load(open(os.path.join(ROOT, "tests", "golden", "poisson_edge_vectors.json")))["poisson"]
    lam = np.array([float.fromhex(r["lambda_hex"]) for r in v])
    got = poisson_log_upper_tail(lam, np.array([r["k"] for r in v], np.int32))
    normal = []
    for r, l, g in zip(v, lam, got):
        if r["band"] != "normal":
            continue
        want = float(r["logp"])
        normal.append(dict(r, lam=float(l), got=float(g), err=abs(float(g) - want) / max(1.0, abs(want))))
    families = []
    for r in v:
        if r["family"] not in families:
            families.append(r["family"])
    out = {"what": "K5 (bdx_poisson_log_upper_tail) against tests/golden/poisson_edge_vectors.json: worst |got - want| / max(1, |want|) "
                   "on log p over the rows whose p is a normal double",
           "per_family": {f: worst([r for r in normal if r["family"] == f]) for f in families},
           "inner_domain": dict(worst([r for r in normal if r["family"] not in ("outer", "grid")]),
                                domain="every family but outer and grid: the series with k <= 8192 and lambda <= 8192 + 3 + 4 sqrt(8192), the closed form of k = 0, lambda <= 0", asserted_bound=1e-10),
           "outer_per_size": {str(n): worst([r for r in normal if r["family"] == "outer" and r["k"] == n]) for n in SIZES},
           "outer_other_points": [worst([r]) for r in normal if r["family"] == "outer" and r["k"] not in SIZES],
           "outer_asserted_bound": 1e-6}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["per_family"]))


if __name__ == "__main__":
    main()
