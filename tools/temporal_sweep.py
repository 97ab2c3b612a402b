"""usage: tools/temporal_sweep.py [out.json]
The sweep behind rf_temporal_default_parameters: a short orbit of the Duck, VIEWS views at 4 samples each (320 x 200, 2 bounces), the fly-camera loop played through
rf_temporal_images over the handle's reads -- accumulate, commit, move -- for every triple of max_history in {16, 32, 64, 128}, depth_tolerance in {0.02, 0.05, 0.1}
and min_normal_dot in {0.8, 0.9, 0.95}.  The error of a triple is the RMSE of T.rgb against a 1024-sample render of the same view, averaged over the views after the
first (which has no history); `plain` is the same figure for the views' own 4-sample means.  Prints JSON: the table, the best triple and the defaults' place in it."""
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
W, H, SPP, TRUTH, BOUNCES, VIEWS = 320, 200, 4, 1024, 2, 6
MAX_HISTORY, DEPTH_TOLERANCE, MIN_NORMAL_DOT = (16.0, 32.0, 64.0, 128.0), (0.02, 0.05, 0.1), (0.8, 0.9, 0.95)


def pose(i):
    """the orbit: 5 degrees of yaw and a stride to the side per view, looking at the Duck"""
    return dict(position=(0.75 - 0.11 * i, 1.0 + 0.01 * i, -0.75 - 0.09 * i), yaw_degrees=129.64 - 5.5 * i, pitch_degrees=-13.73)


def main(out_path):
    import rayfinder_amd as rf
    pt = rf.PtFormat.from_gltf(os.path.join(ROOT, "tests", "golden", "Duck.glb"))
    views = []
    for i in range(VIEWS):
        cam = rf.fly_camera(W, H, **pose(i))
        r = rf.ReferencePathTracer(rf.make_render_parameters(W, H, cam, TRUTH, BOUNCES, rf.make_sky(), 0.25), pt.scene())
        r.set_aovs(True)
        r.render(SPP)
        S, n = r.read_accumulation()
        a = r.read_aovs()
        AC = np.concatenate([a["albedo"], a["coverage"][..., None]], -1)
        ND = np.concatenate([a["normal"], a["depth"][..., None]], -1)
        r.render(TRUTH - SPP)
        full, m = r.read_accumulation()
        assert (n, m) == (SPP, TRUTH)
        views.append(dict(S=S, AC=AC, ND=ND, camera=rf.camera_to_array(cam), truth=full[..., :3].astype(np.float64) / TRUTH))
        r.close()

    def rmse(a, v):
        return float(np.sqrt(np.mean((a.astype(np.float64) - v["truth"]) ** 2)))

    plain = float(np.mean([rmse(v["S"][..., :3] / np.float32(SPP), v) for v in views[1:]]))
    table = []
    for mh, dt, mn in itertools.product(MAX_HISTORY, DEPTH_TOLERANCE, MIN_NORMAL_DOT):
        history, errors, took = None, [], []
        for v in views:
            got = rf.temporal_images(v["S"], v["AC"], v["ND"], SPP, v["camera"], history=history, max_history=mh, depth_tolerance=dt, min_normal_dot=mn)
            if history is not None:
                errors.append(rmse(got["color"][..., :3], v))
                took.append(float((got["color"][..., 3] > SPP).mean()))
            history = dict(color=got["color"], geometry=got["geometry"], camera=v["camera"])
        table.append(dict(max_history=mh, depth_tolerance=dt, min_normal_dot=mn, rmse=round(float(np.mean(errors)), 5), rmse_last_view=round(errors[-1], 5),
                          pixels_with_history=round(float(np.mean(took)), 4)))
    table.sort(key=lambda row: row["rmse"])
    d = rf.temporal_defaults()
    place = next(i for i, row in enumerate(table) if (row["max_history"], row["depth_tolerance"], row["min_normal_dot"]) ==
                 (d["max_history"], round(float(d["depth_tolerance"]), 4), round(float(d["min_normal_dot"]), 4)))
    out = dict(frame=[W, H], views=VIEWS, samples_per_view=SPP, truth_samples=TRUTH, plain_rmse=round(plain, 5), best=table[0], defaults=table[place], defaults_place=place + 1,
               of=len(table), table=table)
    text = json.dumps(out, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
