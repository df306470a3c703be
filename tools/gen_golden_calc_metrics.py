#!/usr/bin/env python3
"""
Golden vectors for the reduce step of calc_metrics.  Dev container only, like gen_golden_eval_approx.py.  The reference's
eval/calc_metrics.py is run UNMODIFIED with --reduce_only (runpy, sys.argv set; tools/_shims holds empty stand-ins for the
skimage.measure, lpips and imageio it imports at the top and uses in its map step alone) on three small made-up render roots:
    plain      three objects, a folder starting with "_" and a stray file
    multicat   --multicat with a metadata file of four categories, one of them without an object
    dtu_sort   --dtu_sort on scan<N> folders whose numeric and lexical orders differ
Its map step cannot run here (it moves tensors to cuda:<id> and needs the lpips package), so only the reduce is pinned.
tests/golden/calc_metrics_reduce.npz holds, per case <c>:
    <c>__objects      (n,) str   the folder names under the render root
    <c>__metrics      (n,) str   the contents of each folder's metrics.txt
    <c>__metadata     str        the contents of the metadata file ("" when the case has none)
    <c>__all_metrics  (m,) uint8 the bytes of the all_metrics.txt the script wrote
and `cases`, the case names.

    python tools/gen_golden_calc_metrics.py
"""
import contextlib
import io
import json
import os
import runpy
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: F401,E402  (puts the reference + shims + tests on sys.path)
import golden_util as gu  # noqa: E402

SCRIPT = os.path.join(os.path.dirname(gen_golden.REF), "eval", "calc_metrics.py")
METADATA = {"02691156": {"id": "02691156", "name": "airplane,aeroplane,plane"}, "02958343": {"id": "02958343", "name": "car,auto"},
            "03001627": {"id": "03001627", "name": "chair"}, "04530566": {"id": "04530566", "name": "vessel,watercraft"}}
CASES = {
    "plain": (["a3f1", "b772", "c0de", "_vis"], []),
    "multicat": (["02691156_1a04e3eab45ca15dd86060f189eb133", "02691156_ffccda82ecc0d0f71740529c616cd4c7",
                  "03001627_u1", "03001627_u2", "03001627_u3", "04530566_e3f6"], ["--multicat", "--metadata", "metadata.yaml"]),
    "dtu_sort": (["scan8", "scan21", "scan103", "scan114", "scan30"], ["--dtu_sort"]),
}


def main():
    rng = np.random.default_rng(20240607)
    out = {"cases": np.array(list(CASES))}
    for case, (objects, flags) in CASES.items():
        with tempfile.TemporaryDirectory() as tmp:
            datadir, output = os.path.join(tmp, "data"), os.path.join(tmp, "render")
            os.makedirs(datadir)
            os.makedirs(output)
            metadata = ""
            if "--multicat" in flags:
                metadata = json.dumps(METADATA, indent=1)
                open(os.path.join(datadir, "metadata.yaml"), "w").write(metadata)
            texts = []
            for obj in objects:
                os.makedirs(os.path.join(output, obj))
                texts.append("psnr {}\nssim {}\nlpips {}".format(float(rng.uniform(18.0, 34.0)), float(rng.uniform(0.7, 0.99)),
                                                                 float(rng.uniform(0.05, 0.3))))
                if not obj.startswith("_"):
                    open(os.path.join(output, obj, "metrics.txt"), "w").write(texts[-1])
            open(os.path.join(output, "finish.txt"), "w").write("a3f1 1.0 1.0 1\n")            # a file, not an object
            argv = sys.argv
            sys.argv = [SCRIPT, "-D", datadir, "-O", output, "--reduce_only"] + flags
            try:
                with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                    runpy.run_path(SCRIPT, run_name="__main__")
            finally:
                sys.argv = argv
            written = open(os.path.join(output, "all_metrics.txt"), "rb").read()
        out[f"{case}__objects"] = np.array(objects)
        out[f"{case}__metrics"] = np.array(texts)
        out[f"{case}__metadata"] = np.array(metadata)
        out[f"{case}__all_metrics"] = np.frombuffer(written, np.uint8)
        print(case)
        print(written.decode())
    path = os.path.join(gu.GOLDEN_DIR, "calc_metrics_reduce.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
