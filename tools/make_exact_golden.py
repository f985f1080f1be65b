#!/usr/bin/env python3
"""Regenerate the option-1 goldens under tests/golden/ and their manifest, tests/golden/exact_manifest.json.

Runs the genuine reference binary (oracle/_ref/Force2Vec -option 1, built by oracle/build_ref.sh where the reference's sources
exist) on the graphs of tests/golden/ and stores the .embd text it wrote, gzipped.  No newly committed file may be larger than 1 MiB
(the older cora goldens beside these, 1.28-1.31 MB each, predate that rule), so a text whose gzip would pass PART_BYTES is stored in
parts of whole lines; the parts, concatenated, are the text, and the manifest's md5 is that of the whole.  Then measures, on the CPU, the
largest absolute difference between the engine-order restatement (tests/exact_ref.py, order="engine") and each golden and records
it: the tests allow four times that value.

Usage: python tools/make_exact_golden.py            (from the repository root)
       python tools/make_exact_golden.py --measure  (keep the files, measure and record the differences again)
"""
import gzip
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exact_ref as R  # noqa: E402
from oracle import oracle as O  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MANIFEST = os.path.join(GOLD, "exact_manifest.json")
PART_BYTES = 1000000  # a gzipped part stays below this

# (graph, epochs, batch, dim, what it covers)
CASES = [
    ("karate.mtx", 5, 16, 16, "baseline"),
    ("karate.mtx", 10, 7, 100, "D not a power of two, partial last minibatch"),
    ("cora.mtx", 3, 256, 128, "full graph"),
]


def gz(data):
    import io
    buf = io.BytesIO()
    with gzip.GzipFile(fileobj=buf, mode="wb", mtime=0) as f:
        f.write(data)
    return buf.getvalue()


def parts_of(text):
    """The text cut at line ends into the fewest equal runs of lines whose gzip stays below PART_BYTES."""
    lines = text.splitlines(keepends=True)
    k = 1
    while True:
        per = (len(lines) + k - 1) // k
        parts = [b"".join(lines[p:p + per]) for p in range(0, len(lines), per)]
        packed = [gz(p) for p in parts]
        if all(len(p) < PART_BYTES for p in packed):
            return packed
        k += 1


def golden_text(case):
    return b"".join(gzip.open(os.path.join(GOLD, f), "rb").read() for f in case["files"])


def main():
    measure_only = "--measure" in sys.argv
    if measure_only:
        manifest = json.load(open(MANIFEST))
    else:
        manifest = {"generator": "tools/make_exact_golden.py", "reference": "oracle/_ref/Force2Vec -option 1 -threads 1", "cases": []}
        for g, iters, batch, dim, covers in CASES:
            with tempfile.TemporaryDirectory() as td:
                path, _ = O.run_reference(os.path.join(GOLD, g), td, 1, iters, batch, dim, threads=1)
                text = open(path, "rb").read()
                name = "%s_opt1_it%d_B%d_D%d" % (g.replace(".mtx", ""), iters, batch, dim)
                packed = parts_of(text)
                files = []
                for k, p in enumerate(packed):
                    files.append(name + (".embd.gz" if len(packed) == 1 else ".part%d.embd.gz" % k))
                    open(os.path.join(GOLD, files[-1]), "wb").write(p)
                manifest["cases"].append({"name": name, "graph": g, "option": 1, "iters": iters, "batch": batch, "dim": dim, "covers": covers,
                                          "md5": hashlib.md5(text).hexdigest(), "embd_name": os.path.basename(path), "files": files})
                print(name, files, [len(p) for p in packed])
    for case in manifest["cases"]:
        rowptr, colids = O.read_mtx(os.path.join(GOLD, case["graph"]))
        with tempfile.NamedTemporaryFile(suffix=".embd") as f:
            f.write(golden_text(case))
            f.flush()
            want = O.read_embd(f.name)
        X0 = O.Rng(1).init_embeddings(len(rowptr) - 1, case["dim"], 0)  # srand(1), randInitF
        got = R.train(X0, rowptr, colids, case["batch"], case["iters"], order="engine")
        case["engine_order_max_abs_diff"] = float(np.abs(got.astype(np.float64) - want).max())
        case["tolerance"] = 4.0 * case["engine_order_max_abs_diff"]
        print(case["name"], "engine order vs golden: max |diff| = %.3g" % case["engine_order_max_abs_diff"])
    with open(MANIFEST, "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
