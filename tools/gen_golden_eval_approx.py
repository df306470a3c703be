#!/usr/bin/env python3
"""
Golden vectors for the view draws of the approximate evaluation.  Dev container only, like gen_golden_video.py.  The
reference's eval/eval_approx.py cannot be imported (it parses arguments, loads a checkpoint and renders), so its three
view-drawing statements are taken out of the loop body of its syntax tree (:111-118) —
    the `if random_source` statement, the `dest_view = torch.randint(..)` assignment, the `for i in range(NS)` loop
— and executed UNMODIFIED, batch after batch after one torch.random.manual_seed(seed) (:89), for the table of cases below.
Only the integer arrays they produce go into tests/golden/eval_approx_views.npz:
    cases              (n, 4) int64: SB, NV, seed, n_batches
    case<i>__source    (NS,) int64, the parsed --source of case i (:96)
    case<i>__src_view  (n_batches, SB, NS) int64
    case<i>__dest_view (n_batches, SB, 1) int64

    python tools/gen_golden_eval_approx.py
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: F401,E402  (puts the reference + shims + tests on sys.path)
import golden_util as gu  # noqa: E402

# SB, NV, source, seed, n_batches
CASES = [(4, 6, "0 2 5", 1234, 2),       # the documented case: dest_view [1, 1, 1, 4] then [4, 3, 1, 1]
         (3, 5, "-1", 7, 3),             # a random source view per object
         (4, 4, "1", 42, 2),             # one fixed source view
         (5, 4, "0 1 3", 99, 2),         # NV - NS = 1: the one view that is left
         (4, 2, "-1", 5, 2),             # NV - NS = 1 with a random source
         (2, 9, "0 1 2 3 4 5 6 7", 1234, 4)]


def view_statements():
    """The three statements, as one module that can be compiled: found in the body of the script's `for data in ..` loop."""
    src = open(os.path.join(os.path.dirname(gen_golden.REF), "eval", "eval_approx.py")).read()
    loops = [n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.For) and isinstance(n.target, ast.Name) and n.target.id == "data"]
    assert len(loops) == 1
    picked = []
    for node in loops[0].body:
        is_if = isinstance(node, ast.If) and isinstance(node.test, ast.Name) and node.test.id == "random_source"
        is_draw = (isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name)
                   and node.targets[0].id == "dest_view" and "randint" in ast.dump(node.value))
        is_skip = isinstance(node, ast.For) and "NS" in ast.dump(node.iter) and "dest_view" in ast.dump(node)
        if is_if or is_draw or is_skip:
            picked.append(node)
    assert [type(n) for n in picked] == [ast.If, ast.Assign, ast.For], [type(n) for n in picked]
    return compile(ast.Module(body=picked, type_ignores=[]), "eval_approx.py:111-118", "exec")


def main():
    code = view_statements()
    out = {"cases": np.array([(sb, nv, seed, nb) for sb, nv, _, seed, nb in CASES], np.int64)}
    for i, (SB, NV, source_arg, seed, n_batches) in enumerate(CASES):
        source = torch.tensor(list(map(int, source_arg.split())), dtype=torch.long)      # :96-98
        NS = len(source)
        random_source = NS == 1 and source[0] == -1
        torch.random.manual_seed(seed)                                                   # :89
        src, dest = [], []
        for _ in range(n_batches):
            env = dict(torch=torch, source=source, NS=NS, random_source=random_source, SB=SB, NV=NV)
            exec(code, env)
            src.append(env["src_view"].clone().numpy())
            dest.append(env["dest_view"].clone().numpy())
        out[f"case{i}__source"] = source.numpy()
        out[f"case{i}__src_view"] = np.stack(src).astype(np.int64)
        out[f"case{i}__dest_view"] = np.stack(dest).astype(np.int64)
        print(SB, NV, repr(source_arg), seed, [d.reshape(-1).tolist() for d in dest])
    assert out["case0__dest_view"].reshape(2, 4).tolist() == [[1, 1, 1, 4], [4, 3, 1, 1]]
    path = os.path.join(gu.GOLDEN_DIR, "eval_approx_views.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
