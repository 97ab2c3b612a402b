#!/usr/bin/env python3
"""Record what a GPU handle says when it refuses a call: tests/golden/refusals_parent.json, the reference tests/test_books.py holds the accumulation's books
(rayfinder_amd/csrc/rf_books.cpp) to.  Run on the commit BEFORE a change to the books or their messages, on a machine with a GPU:

    python tools/record_refusals.py [out.json]

Two sets of cases, both over the walks' frame (tests/handle_walk.py):
  walks   every refused call of the 16 seeded walks: per seed, the call's index, the status and rf_last_error_message();
  cases   tests/books_cases.py: per case the last call's status and message, and -- what depends on pixel values -- the per-tile counts every accepted render_adaptive
          left and the frames every accepted render_until rendered, by the call's index.
Nothing is compared here; a case whose last call is accepted, or whose earlier call is refused, is recorded with a "problem" and fails the run at its end."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ["RF_COMM_TRANSPORT"] = "local"           # check_adaptive: a communicator of one rank, no RCCL

import books_cases as bc                            # noqa: E402
import handle_walk as hw                            # noqa: E402
import rayfinder_amd as rf                          # noqa: E402
import test_gpu_handle_walk as g                    # noqa: E402

SCHEDULING = dict(max_paths_in_flight=0, options={})


def play(r, call, keep, comm):
    """One call on the handle -> ("ok", value) | ("refused", status, message)"""
    name = call[0]
    try:
        if name == "set_direct":
            rf.check(rf.lib.rf_renderer_set_direct(r._h, call[1]))
        elif name == "set_tile_shard":
            rf.check(rf.lib.rf_renderer_set_tile_shard(r._h, call[1], call[2]))
        elif name == "denoise_split":
            r.denoise_split()
        elif name == "export_features":
            r.export_features(channels=call[1])
        elif name in ("read_denoised", "read_robust_mean"):
            getattr(r, name)()
        elif name == "check_adaptive":
            assert call[3] == 1
            comm.render_adaptive(r, call[1], call[2])
        else:
            out = g.apply_gpu(r, call, keep)
            return out if out[0] == "ok" else ("refused", g.INVALID, out[1])
        return ("ok", None)
    except rf.RayfinderError as e:
        return ("refused", int(e.status), str(e))


def record_walks():
    walks = {}
    for seed in hw.SEEDS:
        calls, scheduling = hw.walk(seed)
        r, keep, refused = g.new_handle(scheduling), [], []
        try:
            for i, call in enumerate(calls):
                out = play(r, call, keep, None)
                if out[0] == "refused":
                    refused.append(dict(index=i, call=call[0], status=out[1], message=out[2]))
        finally:
            r.close()
        walks[str(seed)] = refused
    return walks


def record_cases():
    comm = rf.TileComm(rf.comm_unique_id(), 0, 1)
    cases = {}
    try:
        for name, calls in bc.CASES.items():
            r, keep, row = g.new_handle(SCHEDULING), [], dict(counts={}, frames={})
            try:
                for i, call in enumerate(calls):
                    out = play(r, call, keep, comm)
                    last = i == len(calls) - 1
                    if (out[0] == "refused") != last:
                        row["problem"] = f"call {i} {call}: {out[:3]}"
                        break
                    if call[0] == "render_adaptive" and not last:
                        row["counts"][str(i)] = [int(c) for c in r.read_tile_samples().reshape(-1)]
                    if call[0] == "render_until" and not last:
                        row["frames"][str(i)] = int(out[1]["frames"])
                if "problem" not in row:
                    row.update(status=out[1], message=out[2])
            finally:
                r.close()
            cases[name] = row
    finally:
        comm.close()
    return cases


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "refusals_parent.json")
    recording = dict(frame=dict(width=hw.W, height=hw.H, spp=hw.SPP, tiles=hw.TILES), invalid_argument=int(g.INVALID), walks=record_walks(), cases=record_cases())
    with open(out, "w") as f:
        json.dump(recording, f, indent=1, sort_keys=True)
        f.write("\n")
    problems = {name: row["problem"] for name, row in recording["cases"].items() if "problem" in row}
    print(f"{sum(len(w) for w in recording['walks'].values())} refused calls of {len(recording['walks'])} walks, {len(recording['cases'])} cases -> {out}")
    if problems:
        sys.exit(f"cases that did not end in their refusal: {problems}")
