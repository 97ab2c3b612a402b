"""GPU: the traversal kernels across scene scale and distance from the origin, bit for bit against the oracle.

The conservative record layouts (half-precision quad, local-grid quad, oct) rest on error bounds whose every term depends on the absolute
size of the coordinates (rf_wide.hpp: the margins, originBound = 4 R + 1, the 1e-18 .. 1e18 gate on 1/d, the +-65504 box of an empty
slot, +-1e30 for an infinite 1/d).  The rest of the suite traces Duck, the atrium and soups of a few units around the origin; here ONE
soup is traced as base * s + t over the table of tests/scale_scenes.py: centred scales from 1e-2 to 1e12, unit-sized and small soups
1e3 .. 1e7 from the origin, single-axis offsets, and a scene of 1e4 x 1 x 30.  tests/test_host_core.py checks on the CPU that no row is
vacuous (oracle hit fraction of the main rays in (0.05, 0.95), hit and miss pixels under both cameras); the same conditions are asserted
here on the oracle's results.  No row of the issue's table had to be replaced."""
import numpy as np
import pytest

import rayfinder_amd as rf
import scale_scenes as ss
from conftest import bits, oracle_scene_from_pt
from oracle import orc
from test_gpu_parity import _renderer

pytestmark = pytest.mark.gpu

MODE_FLAG = {1: "compact", 2: "hot", 3: "quad", 4: "quad_half", 5: "quad_local", 6: "oct"}


def _scene(name):
    pt = ss.soup_pt(ss.triangles(name))
    return pt, pt.arrays()


def _expected_flags(name, nodes):
    """What the row must have, stated from the table and the root box, not from what the builder gave: everything except the half-precision
    records exists at every scale; those exist exactly when the padded root box fits binary16."""
    return {"regular": True, "compact": True, "hot": True, "quad": True, "quad_half": ss.root_fits_binary16(nodes), "quad_local": True, "oct": True}


@pytest.mark.parametrize("name", ss.ROW_NAMES)
def test_query_path_over_the_scale_table(name):
    pt, a = _scene(name)
    nodes, tris = a["bvhNodes"], a["trianglePositionAttributes"]
    flags = rf.check_wide_layouts(nodes)
    assert flags == _expected_flags(name, nodes), flags
    rays, n_main = ss.scene_rays(nodes)
    unit = ss.row(name)[3]
    r, _ = _renderer(pt, 64, 64, 1, 1)
    half_ratio = r.layout_info(4)["quad_half_area_ratio"]
    for tmax in (float(np.float32(10000.0 * unit)), float(np.float32(1.5 * unit)), ss.FLT_MAX):
        with np.errstate(all="ignore"):
            cpu = orc.intersect_bvh_batch(nodes, tris, rays, tmax)
            cpu_vis = orc.shadow_batch(nodes, tris, rays, tmax)
        frac = float(cpu["hit"][:n_main].mean())
        print(name, "flags", flags, "area ratio", half_ratio, "tmax", tmax, "oracle hit fraction (main rays)", round(frac, 4), "occluded (all rays)", round(float((cpu_vis == 0).mean()), 4))
        if tmax == ss.FLT_MAX:
            assert 0.05 < frac < 0.95, (name, frac)
        r.set_option("query_variant", 2)
        r.set_option("dense_leaf_min", 2)                  # the soup has leaves of three and of twelve triangles: the dense leaf phase runs where a layout has one
        for mode in (0, 1, 2, 3, 4, 5, 6):
            # a mode whose records the scene does not have falls back to the binary records inside the renderer: it is traced all the same, and WHICH modes those are
            # is pinned by the flags asserted above (mode 4 beyond binary16, nothing else)
            assert mode == 0 or flags[MODE_FLAG[mode]] or (mode == 4 and not ss.root_fits_binary16(nodes)), (name, mode)
            r.set_option("query_compact", mode)
            gpu = r.intersect_rays(rays, tmax)
            bad = np.flatnonzero((gpu["hit"] != cpu["hit"]) | (gpu["tri"] != cpu["tri"]))
            assert bad.size == 0, (name, "mode", mode, tmax, "rays", bad[:8], rays[bad[:3]], gpu["tri"][bad[:8]], cpu["tri"][bad[:8]])
            for k in ("t", "uv", "p"):
                assert np.array_equal(bits(gpu[k]), bits(cpu[k])), (name, "mode", mode, tmax, k)
            for nearest_first in (1, 0):
                r.set_option("shadow_nearest_first", nearest_first)
                vis = r.occluded_rays(rays, tmax)
                bad = np.flatnonzero(vis != cpu_vis)
                assert bad.size == 0, (name, "mode", mode, "nearest_first", nearest_first, tmax, "rays", bad[:8], rays[bad[:3]])
            r.set_option("shadow_nearest_first", 1)
        r.set_option("query_compact", 0)
        r.set_option("query_variant", 0)
        gpu = r.intersect_rays(rays, tmax)
        assert np.array_equal(gpu["hit"], cpu["hit"]) and np.array_equal(gpu["tri"], cpu["tri"]), (name, "variant 0", tmax)
        for k in ("t", "uv", "p"):
            assert np.array_equal(bits(gpu[k]), bits(cpu[k])), (name, "variant 0", tmax, k)
        assert np.array_equal(r.occluded_rays(rays, tmax), cpu_vis), (name, "variant 0", tmax)
    assert r.stats()["abandoned_rays"] == 0
    r.close()


FORCED = {"quad_half": dict(quad_half_from_bounce=1, quad_half_shadow_from_bounce=1, quad_local_from_bounce=0, quad_local_shadow_from_bounce=0),
          "quad_local": dict(quad_half_from_bounce=0, quad_half_shadow_from_bounce=0, quad_local_from_bounce=1, quad_local_shadow_from_bounce=1),
          "oct": dict(oct_from_bounce=1)}


@pytest.mark.parametrize("name", ss.ROW_NAMES)
def test_render_path_over_the_scale_table(name):
    pt, a = _scene(name)
    nodes = a["bvhNodes"]
    flags = rf.check_wide_layouts(nodes)
    assert flags == _expected_flags(name, nodes), flags
    ratio = rf.wide_layout_stats(nodes)["quad_half_area_ratio"]
    sc, _ = oracle_scene_from_pt(pt)
    (W, H), spp, bounces = ss.FRAME, 3, 4
    for label, cam, inside in ss.cameras(nodes, W, H):
        c19 = rf.camera_to_array(cam)
        primary = np.array([orc.generate_camera_ray(c19, (x + 0.5) / W, (y + 0.5) / H) for y in range(H) for x in range(W)], np.float32).reshape(-1, 6)
        with np.errstate(all="ignore"):
            hit = orc.intersect_bvh_batch(nodes, a["trianglePositionAttributes"], primary, ss.FLT_MAX)["hit"]
        assert 0 < hit.sum() < hit.size, (name, label, "the oracle's frame has no hit pixel or no miss pixel")
        ref = None
        for forced in (None, "quad_half", "quad_local", "oct"):
            if forced is not None and not flags[forced]:
                assert forced == "quad_half" and not ss.root_fits_binary16(nodes), (name, forced)    # only the half-precision records may be absent, and only beyond binary16
                continue
            r, params = _renderer(pt, W, H, spp, bounces, cam=cam)
            for k, v in (FORCED[forced] if forced else {}).items():
                r.set_option(k, v)
            li = r.layout_info(bounces)
            if forced is None:
                # (a) no option set: what the renderer picked by itself must follow from the flags and the area ratio (rf_wide.hpp: kQuadHalfMaxAreaRatio = 1.075)
                assert li["quad_half_area_ratio"] == pytest.approx(ratio if flags["quad_half"] else 0.0, rel=1e-6), (li, ratio)
                half_ok = flags["quad_half"] and ratio <= 1.075
                print(name, label, "flags", flags, "area ratio", ratio, "closest", li["closest"], "shadow", li["shadow"], "oracle primary hit fraction", round(float(hit.mean()), 4))
                if not half_ok:
                    assert "quad_half" not in li["closest"] + li["shadow"], li
                    assert all(x in ("quad", "quad_local") for x in li["closest"] + li["shadow"]) and "quad_local" in li["closest"], li
                else:
                    assert all(x == "quad_half" for x in li["closest"][1:]), li
                    assert li["closest"][0] == ("quad_half" if inside else "quad"), li
            else:
                # (b) forced from bounce 1; a camera beyond the origin bound keeps its primary launch on the exact quad records (primaryOutside)
                assert all(x == forced for x in li["closest"][1:]), (forced, li)
                assert li["closest"][0] == (forced if inside else "quad"), (forced, li)
                if forced != "oct":
                    assert all(x == forced for x in li["shadow"]), (forced, li)
            r.render(spp)
            img, acc = r.read_accumulation()
            assert acc == spp
            assert r.stats()["abandoned_rays"] == 0
            r.close()
            if ref is None:
                rp = orc.make_render_params(W, H, c19, spp, bounces, 0.25, rf.aligned_sky_state(params.sky))
                with np.errstate(all="ignore"):
                    ref, _ = orc.render(sc, rp, 0, spp)
            g, c = img[..., :3], ref[..., :3]
            assert np.array_equal(np.isnan(g), np.isnan(c)), (name, label, forced, "NaN pixels differ")
            same = (bits(g) == bits(c)) | np.isnan(g)
            with np.errstate(all="ignore"):
                assert same.all(), (name, label, forced, int((~same).sum()), float(np.nanmax(np.abs(g - c))))
