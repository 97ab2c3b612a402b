"""Records tests/golden/launch_plan_parent.json: what the PARENT of the planBatch / planBounce commit launches, over the matrix of tests/test_gpu_launch_plan.py.

Run on the MI355X against a library built from a scratch checkout of the parent commit with profiles/plan/parent_capture.patch applied (it prints one line per
launch, at the launch sites, into the file RF_CAPTURE_FILE names):

    PYTHONPATH=<the parent checkout> RAYFINDER_AMD_LIB=<that library> python profiles/plan/record_parent.py <out.json> [<raw lines out>]

(the parent's Python package: this commit's binds rf_renderer_launch_plan, which the parent's library does not export; the matrix comes from this commit's tests/).

Every cell of the matrix gets fresh handles: one per sample count for the cold state (the batch recorded is the handle's first), one per sample count for the warm
state (a 2-sample render, then the batch recorded).  The lines of the recorded batch are reworded into the fields of rf_launch_plan, one row per bounce."""
import json
import os
import sys
import tempfile

sys.path.append(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))

import rayfinder_amd as rf  # noqa: E402
import test_gpu_launch_plan as m  # noqa: E402

FIELDS = list(rf.ReferencePathTracer.LAUNCH_PLAN_FIELDS) if hasattr(rf.ReferencePathTracer, "LAUNCH_PLAN_FIELDS") else None
KERNEL = {"scalar": 0, "packet": 1, "wide": 2}
ACC = {"plain": 0, "runs": 1, "tiles": 2}


def parse(lines):
    out = []
    for line in lines:
        kind, *kv = line.split()
        d = {k: v for k, v in (x.split("=") for x in kv)}
        out.append((kind, {k: (v if k == "kernel" else int(v)) for k, v in d.items()}))
    return out


def traversal(prefix, kind, d):
    wide = kind == "wide"
    row = {"kernel": KERNEL[kind], "layout": d["compact"] if wide else (7 if kind == "scalar" else 8), "counting": d.get("count", 0), "nearest": d["nearest"] if wide else 0,
           "dense": d["dense"] if wide else 0, "refill_min": d["refill"] if wide else 0, "chunk": d["chunk"] if wide else 0, "leaf_vote": d["vote"] if wide else 0,
           "flags": d["flags"], "extra_lds": d["extraLds"] if wide else 0, "count_word": d["countWord"], "cursor_word": d["cursorWord"] if wide else 0}
    return {prefix + k: v for k, v in row.items()}


def plans_of(lines, bounces):
    recs = parse(lines)
    one = lambda kind: [d for k, d in recs if k == kind]
    batch, raygen, acc = one("batch")[0], one("raygen")[0], one("acc")[0]
    assert len(one("batch")) == 1 and len(one("acc")) == 1, "more than one batch was recorded"
    rows = []
    for b in range(1, bounces + 1):
        mine = [(k, d) for k, d in recs if d.get("bounce") == b]
        closest = [(k, d) for k, d in mine if k in KERNEL and d["anyHit"] == 0]
        shadow = [(k, d) for k, d in mine if k in KERNEL and d["anyHit"] == 1]
        shade = [d for k, d in mine if k == "shade"]
        look = [d for k, d in mine if k == "look"]
        assert len(closest) == 1 and len(shadow) == 1 and len(shade) == 1 and len(look) <= 1, (b, mine)
        first = [(k, d) for k, d in recs if k in KERNEL and d.get("bounce") == 1 and d["anyHit"] == 0][0]
        row = dict(num_samples=batch["numSamples"], num_bounces=batch["numBounces"], sample_perm=batch["samplePerm"], dense_raygen=raygen["denseRaygen"],
                   const_origin=raygen["skipOrigins"], primary_layout=traversal("", *first)["layout"], occluder_grid=raygen["occGrid"], occluder_scale_bits=raygen["occScale"],
                   occluder_mask=raygen["occMask"], runs=acc["runs"], tile_list=int(acc["kernel"] == "tiles"), accumulate_kernel=ACC[acc["kernel"]], accumulate_pixels=acc["pixels"],
                   aov_pixels=(one("accaov") or [{"pixels": 0}])[0]["pixels"], moment_pixels=(one("accmoments") or [{"pixels": 0}])[0]["pixels"], raygen_count_word=raygen["countWord"])
        row.update(traversal("closest_", *closest[0]))
        s = shade[0]
        row.update(shade_sorted=s["sorted"], shade_aov=s["aov"], shade_flags=s["flags"], shade_sort_scale=s["sortScale"], shade_grid_cap=0 if s["grid"] == s["itemBlocks"] else s["grid"])
        row.update(traversal("shadow_", *shadow[0]))
        kind, d = shadow[0]
        row.update(shadow_cached=int(bool(d["flags"] & 16)) if kind == "wide" else 0, shadow_first_look=len(look), shadow_self=int(bool(s["flags"] & 4)),
                   shadow_source=d["rayList"] if kind == "wide" else 0, look_flags=look[0]["flags"] if look else 0, look_count_word=look[0]["inCountWord"] if look else 0,
                   look_list_word=look[0]["listCountWord"] if look else 0)
        rows.append(row)
    return rows


def pack(fields, plans):
    """The recording as a few hundred short records: the distinct once-per-batch rows and the distinct per-bounce rows, one per line, and per cell of the matrix the
    rows of its bounces (they do not depend on the sample count) and the batch row of each sample count.  tests/test_gpu_launch_plan.py puts them together again."""
    split = fields.index("closest_kernel")
    batch_rows, bounce_rows, cells = [], [], {}
    index = lambda table, row: table.index(row) if row in table else (table.append(row) or len(table) - 1)
    for key, rows in plans.items():
        cell, n = key.rsplit("/", 1)
        bounces = [index(bounce_rows, row[split:]) for row in rows]
        assert all(row[:split] == rows[0][:split] for row in rows)
        c = cells.setdefault(cell, {"bounces": bounces, "batch": {}})
        assert c["bounces"] == bounces, "the bounces' rows depend on the sample count: keep them per sample count"
        c["batch"][n] = index(batch_rows, rows[0][:split])
    line = lambda v: json.dumps(v, separators=(",", ":"))
    table = lambda rows: "[\n" + ",\n".join(line(r) for r in rows) + "\n]"
    return ("{\n" + f'"batch_fields":{line(fields[:split])},\n"bounce_fields":{line(fields[split:])},\n"batch_rows":{table(batch_rows)},\n"bounce_rows":{table(bounce_rows)},\n'
            + '"cells":{' + ",".join(("\n" if k.endswith("/" + m.STATES[0]) else "") + f"{line(k)}:{line(v)}" for k, v in cells.items()) + "\n}\n}\n")


def main():
    out_path = sys.argv[1]
    raw = {}
    plans = {}
    fields = FIELDS
    cap = os.path.join(tempfile.mkdtemp(), "capture.txt")
    for scene, case in m.MATRIX:
        for state in m.STATES:
            for n in m.SAMPLE_COUNTS:
                r = m.make_handle(scene, case)
                if state == "warm":
                    r.render(2)
                    r.synchronize()
                if os.path.exists(cap):
                    os.remove(cap)
                os.environ["RF_CAPTURE_FILE"] = cap
                r.render(n)
                r.synchronize()
                del os.environ["RF_CAPTURE_FILE"]
                r.close()
                with open(cap) as f:
                    lines = [x.strip() for x in f if x.strip()]
                key = f"{scene}/{case}/{state}/{n}"
                raw[key] = lines
                rows = plans_of(lines, m.BOUNCES)
                if fields is None:
                    fields = list(rows[0])
                plans[key] = [[row[k] for k in fields] for row in rows]
        print(scene, case, "recorded", flush=True)
    with open(out_path, "w") as f:
        f.write(pack(fields, plans))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(raw, f, indent=0)
    print("cells:", len(plans))


if __name__ == "__main__":
    main()
