"""A reference model of ONE renderer handle's bookkeeping, written from include/rayfinder_amd.h alone: pure Python and numpy over the CPU oracle, composing the
restatements the kernel tests already trust (adaptive_restatement, noise_restatement, aov_restatement, denoise*_restatement, robust*_restatement).  It imports nothing
of the product but the tile deal (rf.tiles_for_rank, host arithmetic).

Every observable of a handle is an exact function of the call sequence and of the per-sample radiance and first-hit records of the samples traced.  The model keeps
the sequence's state -- the frame counter, the accumulated (leading) count L, the per-tile counts, and for each family of sums (S; Q; AC / ND; the K bucket planes)
the ordinal of the accumulation's sample from which it has been on -- and forms every sum, when it is read, from the oracle's samples:

    sample i of an accumulation is the absolute frame first_frame + i (the frame counter when the accumulation started; rf_renderer_render traces frameCount,
    frameCount + 1, ...), tile t holds samples 0 .. counts[t] - 1, and a family that has been on since sample `start` sums samples start .. counts[t] - 1 of tile t,
    in sample order from +0 (the buckets: sample j of those in plane j mod K).

The per-sample cache is keyed by the ABSOLUTE frame number (the oracle's radiance of frame f is not that of frame f + spp) and shared by every model of a process.

Every method mirrors one call and returns ("ok", value) or ("refused", keyword).  The keyword is what the header promises about the message, as a tuple of strings
(None: nothing promised).  Where several refusals apply and the header states no order among them, the model promises only what ALL of them promise.  A refused
call changes nothing.  Rules the header leaves open are decided from its general rules (a sum covers the accumulation only if it was on from the first sample;
whatever clears the image clears every sum, both per-tile states and both snapshots) and are written into the header, never taken from the product."""
import numpy as np

from adaptive_restatement import estimate_tiles, mean_image, play, tile_slices
from aov_restatement import first_hit_samples
from denoise_restatement import denoise
from denoise_tiles_restatement import denoise_tiles
from noise_restatement import estimate
from oracle import orc
from robust_restatement import denoise_robust, robust_mean
from robust_tiles_restatement import denoise_robust_tiles, robust_mean_tiles

AOV_FIRST_HIT, AOV_TILE_COUNTS, BUCKETS_TILE_COUNTS = 0x1, 0x100, 0x100
NON_UNIFORM = ("different sample counts",)
RESTART = ("restart the accumulation first",)
BUCKET = ("bucket",)
F = np.float32

_SAMPLES = {}        # (frame setup, absolute frame) -> (H, W, 3) f32 radiance of that one sample
_RECORDS = {}        # (frame setup, absolute frame) -> ((H, W, 4), (H, W, 4)) f32 first-hit records {albedo.rgb, coverage}, {normal.xyz, depth}
_SCENES = []         # (the scenes whose id() is part of a key stay alive)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(x):
    return int(np.float64(x).view(np.uint64))


def ok(value=None):
    return ("ok", value)


def refused(reasons):
    """reasons: the keyword tuples (or None) of every refusal that applies -> what all of them promise"""
    common = None
    for i, r in enumerate(reasons):
        words = set(r or ())
        common = words if i == 0 else common & words
    return ("refused", tuple(sorted(common)) or None)


def estimate_scalars(e):
    """The scalars of an estimate as integers / bit patterns (None: no estimate was made)"""
    if e is None:
        return None
    return dict(mean_error=bits64(e["mean_error"]), max_error=int(bits(F(e["max_error"])).reshape(-1)[0]), worst_tile=int(e["worst_tile"]), samples=int(e["samples"]),
                pixels=int(e["pixels"]), nonfinite_pixels=int(e["nonfinite_pixels"]))


class _Prefix:
    """S[n], Q[n] for play(): the sums of the accumulation's first n samples, formed on demand (a call that stops early never asks the oracle for later frames)"""

    def __init__(self, model, square):
        self.model, self.square = model, square

    def __getitem__(self, n):
        return self.model._sum("Q" if self.square else "S", 0, int(n))


class HandleModel:
    def __init__(self, scene, width, height, spp, bounces, exposure, camera, sky):
        self.scene, self.w, self.h, self.spp, self.bounces = scene, width, height, spp, bounces
        self.camera, self.sky = np.array(camera, np.float32), np.array(sky, np.float32)
        self.exposure = float(F(exposure))
        self.rp = orc.make_render_params(width, height, self.camera, spp, bounces, self.exposure, self.sky)
        if not any(s is scene for s in _SCENES):
            _SCENES.append(scene)
        self._key = (id(scene), width, height, spp, bounces, self.camera.tobytes(), self.sky.tobytes())
        self.slices = tile_slices(width, height)
        self.tiles = len(self.slices)
        self.pixels = [(r.stop - r.start) * (c.stop - c.start) for r, c in self.slices]
        self.frame_count = 0
        self.rank, self.world = 0, 1
        self.own = list(range(self.tiles))          # the tiles of the shard
        self.bound = False
        self.moments_on, self.aov_flags, self.K, self.bucket_bit = False, 0, 0, False
        self.primary_rays = 0
        self.frames_traced = set()                  # absolute frames this handle traced (the CPU test bounds them)
        self._sums = {}
        self._restart()

    # ---- the samples -------------------------------------------------------------------------------------------------------------------------------------------
    def _radiance(self, frame):
        key = (self._key, int(frame))
        if key not in _SAMPLES:
            image = np.zeros((self.h, self.w, 4), np.float32)
            orc.render(self.scene, self.rp, int(frame), 1, image=image, accumulated_start=0)        # 0 + r = r: the sample alone
            _SAMPLES[key] = image[..., :3].copy()
            _SAMPLES[key].setflags(write=False)
        return _SAMPLES[key]

    def _records(self, frame):
        key = (self._key, int(frame))
        if key not in _RECORDS:
            ys, xs = np.mgrid[0:self.h, 0:self.w]
            ac, nd = first_hit_samples(self.scene, self.rp, xs.ravel(), ys.ravel(), int(frame))
            _RECORDS[key] = (ac.reshape(self.h, self.w, 4), nd.reshape(self.h, self.w, 4))
            for a in _RECORDS[key]:
                a.setflags(write=False)
        return _RECORDS[key]

    def _sum(self, kind, start, stop):
        """The whole frame's sum of samples start .. stop - 1 of this accumulation, in sample order from +0.  kind: S, Q (H, W, 4), AC, ND (H, W, 4), B (K, H, W, 4).
        Built from the sum up to stop - 1 (the same chain, one addition longer) and kept per accumulation."""
        key = (kind, self.K if kind == "B" else 0, start, stop)
        if key in self._sums:
            return self._sums[key]
        shape = (self.K, self.h, self.w, 4) if kind == "B" else (self.h, self.w, 4)
        if stop <= start:
            out = np.zeros(shape, np.float32)
        else:
            out = self._sum(kind, start, stop - 1).copy()
            frame = self.first_frame + stop - 1
            if kind == "S":
                out[..., :3] = out[..., :3] + self._radiance(frame)
            elif kind == "Q":
                r = self._radiance(frame)
                out[..., :3] = out[..., :3] + r * r
            elif kind == "B":
                b = (stop - 1 - start) % self.K                                                     # the sample's ordinal among the bucket samples, mod K
                out[b, ..., :3] = out[b, ..., :3] + self._radiance(frame)
            else:
                out = out + self._records(frame)[0 if kind == "AC" else 1]
        out.setflags(write=False)
        self._sums[key] = out
        return out

    def _held(self, kind, start):
        """What the handle holds of a family that has been on since sample `start`: tile t from the sum of its samples start .. counts[t] - 1; zeros outside the shard"""
        out = np.zeros((self.K, self.h, self.w, 4) if kind == "B" else (self.h, self.w, 4), np.float32)
        for t in self.own:
            rows, cols = self.slices[t]
            out[..., rows, cols, :] = self._sum(kind, start, int(self.counts[t]))[..., rows, cols, :]
        return out

    # ---- the state ---------------------------------------------------------------------------------------------------------------------------------------------
    def _restart(self):
        """A new accumulation: what clears the image clears every sum with its count, both per-tile states and both snapshots.  The frame counter stays."""
        self.first_frame = self.frame_count
        self.L = 0
        self.counts = np.zeros(self.tiles, np.int64)
        self.q_start = self.a_start = self.b_start = 0
        self.denoised = self.robust = None
        self._sums = {}

    @property
    def accumulated(self):
        return self.L

    def non_uniform(self):
        return any(self.counts[t] != self.L for t in self.own)

    def _aov_on(self):
        return bool(self.aov_flags & AOV_FIRST_HIT)

    def _aov_bit(self):
        return bool(self.aov_flags & AOV_TILE_COUNTS)

    def _count(self, on, start):
        """A family's own sample count: the samples traced while it was on"""
        return self.L - start if on else 0

    def _covers(self, on, start):
        return on and start == 0

    def _trace(self, n, tiles):
        """n more samples of `tiles` (all of them at L): frames frame_count .. frame_count + n - 1"""
        assert self.first_frame + self.L == self.frame_count or n == 0
        self.frames_traced.update(range(self.frame_count, self.frame_count + n))
        for t in tiles:
            self.counts[t] += n
            self.primary_rays += n * self.pixels[t]
        self.L += n
        self.frame_count += n

    # ---- state-changing calls ----------------------------------------------------------------------------------------------------------------------------------
    def render(self, n):
        if self.non_uniform():
            return refused([NON_UNIFORM])
        traced = min(n, self.spp - self.L)
        self._trace(traced, self.own)
        self.frame_count += n - traced                                                              # calls past spp only advance frameCount
        return ok()

    def _estimate_now(self):
        s, q = self._held("S", 0), self._held("Q", self.q_start)
        if self.non_uniform():
            return estimate_tiles(s, q, self.counts, self.w, self.h)
        return estimate(s, q, self.L)

    def render_until(self, target, every, max_frames):
        reasons = []
        if not self.moments_on:
            reasons.append(None)
        if self.non_uniform():
            reasons.append(NON_UNIFORM)
        if self.world != 1:
            reasons.append(None)
        if every == 0:
            reasons.append(None)
        if self.moments_on and self.L != 0 and self.q_start != 0:
            reasons.append(None)
        if reasons:
            return refused(reasons)
        if self.L == 0:
            self.q_start = 0
        frames, last = 0, None
        while frames < max_frames and self.L < self.spp:
            n = min(every, max_frames - frames, self.spp - self.L)
            self._trace(n, self.own)
            frames += n
            if self.L < 2:
                continue
            last = self._estimate_now()
            if last["mean_error"] <= float(F(target)):
                break
        return ok(dict(frames=frames, last=estimate_scalars(last)))

    def render_adaptive(self, target, every, min_samples=0, max_samples=0):
        reasons = []
        if self.K and not self.bucket_bit:
            reasons.append(BUCKET)
        if not self.moments_on:
            reasons.append(None)
        if self._aov_on() and not self._aov_bit():
            reasons.append(None)
        if self.world != 1:
            reasons.append(None)
        if every == 0:
            reasons.append(None)
        if not (np.isfinite(F(target)) and F(target) >= 0):
            reasons.append(None)
        if self.L != 0:
            if self.moments_on and self.q_start != 0:
                reasons.append(RESTART)
            if self._aov_on() and self.a_start != 0:
                reasons.append(RESTART)
            if self.K and self.b_start != 0:
                reasons.append(RESTART)
        if reasons:
            return refused(reasons)
        before = self.counts.copy()
        res = play(_Prefix(self, False), _Prefix(self, True), self.w, self.h, target, every, min_samples=min_samples, max_samples=max_samples, spp=self.spp,
                   counts=self.counts)
        grown = int(res["leading"]) - self.L
        self.frames_traced.update(range(self.frame_count, self.frame_count + grown))
        self.frame_count += grown                                                                   # the frame counter advances by the growth of L
        self.L = int(res["leading"])
        self.counts = np.array(res["counts"], np.int64)
        self.primary_rays += int(sum(p * int(c - b) for p, c, b in zip(self.pixels, self.counts, before)))
        value = {k: int(res[k]) for k in ("estimate_passes", "stopped_tiles", "min_tile_samples", "max_tile_samples", "pixel_samples")}
        value.update(tiles=self.tiles, last=estimate_scalars(res["last"]))
        return ok(value)

    def set_moments(self, on):
        on = bool(on)
        if on != self.moments_on:
            self.moments_on, self.q_start = on, self.L                                              # cleared, the count 0: covers only the later samples
        return ok()

    def set_aovs(self, flags):
        if flags & ~(AOV_FIRST_HIT | AOV_TILE_COUNTS) or (flags & AOV_TILE_COUNTS and not flags & AOV_FIRST_HIT):
            return refused([None])
        if flags != self.aov_flags:                                                                 # any change of the value clears the sums and drops the snapshot
            self.aov_flags, self.a_start, self.denoised = flags, self.L, None
        return ok()

    def set_buckets(self, arg):
        k, bit = arg & 0xFF, bool(arg & BUCKETS_TILE_COUNTS)
        reasons = []
        if arg & ~(0xFF | BUCKETS_TILE_COUNTS) or (k == 0 and arg != 0) or (k != 0 and (k % 2 == 0 or k < 3 or k > 15)):
            reasons.append(None)
        if k != 0 and self.non_uniform():
            reasons.append(NON_UNIFORM)
        if reasons:
            return refused(reasons)
        if k != self.K or bit != self.bucket_bit:                                                   # a change of K or of the bit alone clears the sums and drops the snapshot
            self.K, self.bucket_bit, self.b_start, self.robust = k, bit, self.L, None
        return ok()

    def set_render_parameters(self, exposure):
        exposure = float(F(exposure))
        if exposure != self.exposure:
            self.exposure = exposure
            self.rp = orc.make_render_params(self.w, self.h, self.camera, self.spp, self.bounces, exposure, self.sky)   # (radiance does not depend on it: same cache key)
            self._restart()
        return ok()

    def set_tile_shard(self, rank, world):
        reasons = []
        if world == 0 or rank >= world:
            reasons.append(None)
        if self.non_uniform():
            reasons.append(NON_UNIFORM)
        if reasons:
            return refused(reasons)
        import rayfinder_amd as rf                                                                  # the tile deal: host arithmetic
        self.rank, self.world = rank, world
        self.own = sorted(int(t) for t in rf.tiles_for_rank(self.w, self.h, rank, world))
        self._restart()                                                                             # every accepted call deals the tiles anew and restarts
        return ok()

    def bind_accumulation_buffer(self, bound):
        """bound: True = a caller's buffer (large enough), False = back to the handle's own.  Either restarts the accumulation."""
        self.bound = bool(bound)
        self._restart()
        return ok()

    # ---- queries -----------------------------------------------------------------------------------------------------------------------------------------------
    def noise_estimate(self):
        reasons = []
        if not self.moments_on:
            reasons.append(None)
        if self.world != 1:
            reasons.append(None)
        if self.moments_on and (self.q_start != 0 or self.L == 0):
            reasons.append(None)
        if self.L < 2:
            reasons.append(None)
        if reasons:
            return refused(reasons)
        e = self._estimate_now()
        if self.non_uniform():
            e = dict(e, samples=self.L)
        value = estimate_scalars(e)
        value.update(error_map=bits(e["error_map"]), tile_sum=bits(e["tile_sum"]), tile_max=bits(e["tile_max"]))
        return ok(value)

    def _denoise_reasons(self):
        """rf_renderer_denoise's refusals; the non-uniform state's comes before the others (the header says so), so it alone decides the keyword when it applies"""
        if self.non_uniform() and not (self._aov_on() and self._aov_bit() and self.a_start == 0):
            return [NON_UNIFORM]
        reasons = []
        if not self._aov_on():
            reasons.append(None)
        if self.world != 1:
            reasons.append(None)
        if self.L == 0:
            reasons.append(None)
        if self._aov_on() and self.a_start != 0:
            reasons.append(None)
        return reasons

    def _robust_reasons(self):
        reasons = []
        per_tile = self.non_uniform() and self.K and self.bucket_bit
        if self.non_uniform() and not per_tile:
            reasons.append(NON_UNIFORM)
        if not self.K:
            reasons.append(None)
        if self.world != 1:
            reasons.append(None)
        if self.K and self.L < self.K:
            reasons.append(None)
        if self.K and self.b_start != 0:
            reasons.append(None)
        if per_tile and min(int(self.counts[t]) for t in self.own) < self.K:
            reasons.append((str(self.K), str(min(int(self.counts[t]) for t in self.own))))       # the message names K and the smallest count
        return reasons

    def _texels(self, rgb):
        """kTonemap with accumulatedSamples = 1 and the handle's exposure over {rgb, 1}"""
        rgba = np.concatenate([np.asarray(rgb, np.float32), np.ones((self.h, self.w, 1), np.float32)], -1)
        return orc.tonemap_bgra8(rgba.reshape(-1, 4), 1, self.exposure).reshape(self.h, self.w)

    def denoise(self, iterations=5, sigma_color=1.0, sigma_normal=0.1, sigma_depth=0.1):
        reasons = self._denoise_reasons()
        if reasons:
            return refused(reasons)
        s, ac, nd = self._held("S", 0), self._held("AC", 0), self._held("ND", 0)
        p = dict(iterations=iterations, sigma_color=sigma_color, sigma_normal=sigma_normal, sigma_depth=sigma_depth)
        rgb = denoise_tiles(s, ac, nd, self.counts, **p) if self.non_uniform() else denoise(s, ac, nd, self.L, **p)
        self.denoised = dict(rgb=bits(rgb), bgra=self._texels(rgb), samples=self.L)
        return ok()

    def _combine(self):
        B = self._held("B", 0)
        M, trim = robust_mean_tiles(B, self.counts, self.w, self.h) if self.non_uniform() else robust_mean(B, self.L)
        self.robust = dict(mean=bits(M), trim=trim.astype(np.uint8), bgra=self._texels(M), samples=self.L)
        return M

    def robust_mean(self):
        reasons = self._robust_reasons()
        if reasons:
            return refused(reasons)
        self._combine()
        return ok()

    def denoise_robust(self, iterations=5, sigma_color=1.0, sigma_normal=0.1, sigma_depth=0.1):
        reasons = self._denoise_reasons()
        if reasons != [NON_UNIFORM] or not self.non_uniform():
            reasons = reasons + self._robust_reasons()                                              # refused as denoise is, and also when robust_mean would be
        if reasons:
            return refused(reasons)
        M = self._combine()
        ac, nd = self._held("AC", 0), self._held("ND", 0)
        p = dict(iterations=iterations, sigma_color=sigma_color, sigma_normal=sigma_normal, sigma_depth=sigma_depth)
        rgb = denoise_robust_tiles(M, ac, nd, self.counts, **p) if self.non_uniform() else denoise_robust(M, ac, nd, self.L, **p)
        self.denoised = dict(rgb=bits(rgb), bgra=self._texels(rgb), samples=self.L)
        return ok()

    # ---- reads -------------------------------------------------------------------------------------------------------------------------------------------------
    def read_accumulation(self):
        return self._held("S", 0), self.L

    def read_moments(self):
        return (self._held("Q", self.q_start) if self.moments_on else np.zeros((self.h, self.w, 4), np.float32)), self._count(self.moments_on, self.q_start)

    def read_aovs(self):
        zero = np.zeros((self.h, self.w, 4), np.float32)
        on = self._aov_on()
        return (self._held("AC", self.a_start) if on else zero), (self._held("ND", self.a_start) if on else zero), self._count(on, self.a_start)

    def read_buckets(self):
        return (self._held("B", self.b_start) if self.K else np.zeros((0, self.h, self.w, 4), np.float32)), self.K, self._count(bool(self.K), self.b_start)

    def read_tile_samples(self):
        return self.counts.copy()

    def tile_samples_uniform(self):
        return np.unique(self.counts[self.counts > 0]).size <= 1

    def read_mean(self):
        mean = mean_image(self._held("S", 0), self.counts, self.w, self.h)
        for t in range(self.tiles):
            if t not in self.own:
                rows, cols = self.slices[t]
                mean[rows, cols] = 0                                                                # pixels outside the shard's tiles: four zeros
        return mean

    def read_tonemapped(self):
        texels = orc.tonemap_bgra8(self.read_mean().reshape(-1, 4), 1, self.exposure).reshape(self.h, self.w)
        for t in range(self.tiles):
            if t not in self.own:
                rows, cols = self.slices[t]
                texels[rows, cols] = 0
        return texels

    def read_denoised(self):
        return ok(self.denoised) if self.denoised is not None else refused([None])

    def read_robust_mean(self):
        return ok(self.robust) if self.robust is not None else refused([None])

    def stats(self):
        return dict(primary_rays=self.primary_rays)                                                 # the pixel-samples traced

    def observe(self):
        """Every read as one dict of bit patterns and integers: the comparison surface"""
        s, acc = self.read_accumulation()
        q, qn = self.read_moments()
        ac, nd, an = self.read_aovs()
        b, k, bn = self.read_buckets()
        out = dict(acc=acc, S=bits(s[..., :3]), Q=bits(q), q_n=qn, AC=bits(ac), ND=bits(nd), aov_n=an, B=bits(b), K=k, b_n=bn,
                   counts=self.read_tile_samples(), uniform=bool(self.tile_samples_uniform()), mean=bits(self.read_mean()), bgra=self.read_tonemapped(),
                   primary_rays=self.stats()["primary_rays"], has_denoised=self.denoised is not None, has_robust=self.robust is not None)
        if self.denoised is not None:
            out.update(den_rgb=self.denoised["rgb"], den_bgra=self.denoised["bgra"], den_n=self.denoised["samples"])
        if self.robust is not None:
            out.update(rob_mean=self.robust["mean"], rob_trim=self.robust["trim"], rob_bgra=self.robust["bgra"], rob_n=self.robust["samples"])
        return out


def differing(a, b):
    """The observables that differ between two observe() dicts (a key one side lacks differs)"""
    return [k for k in sorted(set(a) | set(b)) if k not in a or k not in b or not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]
