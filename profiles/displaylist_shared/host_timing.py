"""Host cost of the leaf analysis, for comparing two checkouts: `python host_timing.py ROOT LABEL [--ops]` prints one JSON line.

Per workload [median ms, min ms] of 200 repeats (2 000 for the sub-millisecond one; the first is dropped), or with --ops the
bytecode instructions and Python calls of one repeat (deterministic: what a noisy host cannot resolve in milliseconds).
  walk_*      `_batchable_leaves(scene, tr, lin)` + `_drop_empty` with `STATE.leaf_memo` set as a top-level render sets it
  children_*  the same question asked per child of the root group (`_leaves_memo`): how the walk asks when the whole is not batchable
  compile_material  `displaylist._compile`
Run a fresh interpreter per side, the sides alternating."""
import json
import os
import statistics
import sys
import time

root, label = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, root)
import svgrasterize_amd as S  # noqa: E402
from svgrasterize_amd import displaylist, scene as sc, scenedump  # noqa: E402
from svgrasterize_amd._state import STATE  # noqa: E402

N = 201
count = {"opcode": 0, "call": 0}


def tracer(frame, event, _arg):
    frame.f_trace_opcodes = True
    if event in count:
        count[event] += 1
    return tracer


def measure(fn, n=N):
    if "--ops" in sys.argv:
        fn()
        count["opcode"] = count["call"] = 0
        sys.settrace(tracer)
        try:
            fn()
        finally:
            sys.settrace(None)
        return {"ops": count["opcode"], "calls": count["call"]}
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return [round(statistics.median(ts[1:]) * 1e3, 4), round(min(ts[1:]) * 1e3, 4)]


out = {"label": label}
for name in ("material", "icons4096"):
    scene, info, _pins = scenedump.load_scene(os.path.join(root, "tests", "golden", f"scene_{name}.npz"))
    tr = S.Transform().matrix(0, 1, 0, 1, 0, 0).scale(4096 / info["full"]["size"][0])
    top, ttr = scene, tr
    while top[0] == sc.RENDER_TRANSFORM:
        ttr, top = ttr @ top[1][1], top[1][0]

    def asked(nodes, transform, ask):
        STATE.leaf_memo = {}
        try:
            for node in nodes:
                leaves = ask(node, transform, False)
                if leaves is not None:
                    sc._drop_empty(leaves)
        finally:
            STATE.leaf_memo = None

    out[f"walk_{name}"] = measure(lambda: asked([scene], tr, sc._batchable_leaves), N if name == "material" else 10 * N)
    out[f"children_{name}"] = measure(lambda: asked(top[1], ttr, sc._leaves_memo))
    if name == "material":
        out["compile_material"] = measure(lambda: displaylist._compile(scene, False))
print(json.dumps(out))
