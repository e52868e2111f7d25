"""The deviation map restated on the host: Python integers for the sums (exact S1, S2, n S2 - S1^2 and
float(int), which rounds to nearest, ties to even), numpy float64 for the rest, math.fsum for the floating-point sums.
Regions go through _defect_map_ref.regions' machinery."""
import math

import numpy as np

import _defect_map_ref as dref

Q = 2.0 ** -20
MAX_GATE = 1024.0
FACE_KEYS = ("n", "frames", "s1", "s2_hi", "s2_lo", "min", "max", "mean", "std")
REGION_BIT_COLUMNS = ("min_mean", "max_mean")


def quantise(d):
    """q = rint(d 2^20) as int64, round half to even; the product is exact in float64."""
    return np.rint(np.asarray(d, dtype=np.float64) * 2.0 ** 20).astype(np.int64)


def row_kinds(ids, d, F, gate, backfacing=None):
    """(taken, ignored, gated, back): boolean rows.  Bad id or NaN: ignored; then backfacing; then the gate."""
    ids = np.asarray(ids).astype(np.int64)
    d = np.asarray(d, dtype=np.float64)
    ignored = (ids < 0) | (ids >= F) | np.isnan(d)
    back = ~ignored & (np.zeros(len(d), bool) if backfacing is None else np.asarray(backfacing, dtype=bool))
    with np.errstate(invalid="ignore"):
        inside = np.abs(d) <= gate
    taken = ~ignored & ~back & inside
    gated = ~ignored & ~back & ~inside
    return taken, ignored, gated, back


class State:
    def __init__(self, F):
        self.F = F
        self.n = np.zeros(F, np.int64)
        self.frames = np.zeros(F, np.int32)
        self.s1 = np.zeros(F, np.int64)
        self.s2 = [0] * F                       # Python integers: exact
        self.qmin = np.zeros(F, np.int64)
        self.qmax = np.zeros(F, np.int64)
        self.observations = self.rows_taken = self.rows_ignored = self.rows_gated = self.rows_backfacing = 0

    def add(self, ids, d, gate=MAX_GATE, backfacing=None):
        assert 0.0 <= gate <= MAX_GATE
        ids = np.asarray(ids).astype(np.int64)
        d = np.asarray(d, dtype=np.float64)
        taken, ignored, gated, back = row_kinds(ids, d, self.F, gate, backfacing)
        f, q = ids[taken], quantise(d[taken])
        assert (np.abs(q) <= 2 ** 30).all()
        fresh = np.unique(f[self.n[f] == 0])
        self.qmin[fresh], self.qmax[fresh] = 2 ** 62, -2 ** 62
        np.add.at(self.n, f, 1)
        np.add.at(self.s1, f, q)
        np.minimum.at(self.qmin, f, q)
        np.maximum.at(self.qmax, f, q)
        qq = q * q                              # < 2^61: its two 32-bit halves are summed in int64 without overflow
        lo, hi = np.zeros(self.F, np.int64), np.zeros(self.F, np.int64)
        np.add.at(lo, f, qq & 0xFFFFFFFF)
        np.add.at(hi, f, qq >> 32)
        for face in np.unique(f):
            self.s2[face] += (int(hi[face]) << 32) + int(lo[face])
        self.frames[np.unique(f)] += 1
        self.observations += 1
        self.rows_taken += int(taken.sum())
        self.rows_ignored += int(ignored.sum())
        self.rows_gated += int(gated.sum())
        self.rows_backfacing += int(back.sum())
        return self

    def faces(self):
        F = self.F
        out = {"n": self.n.copy(), "frames": self.frames.copy(), "s1": self.s1.copy(),
               "s2_hi": np.array([s >> 64 for s in self.s2], dtype=np.uint64).reshape(F),
               "s2_lo": np.array([s & (2 ** 64 - 1) for s in self.s2], dtype=np.uint64).reshape(F)}
        for k in ("min", "max", "mean", "std"):
            out[k] = np.full(F, np.nan)
        for f in np.nonzero(self.n)[0]:
            n, s1, s2 = int(self.n[f]), int(self.s1[f]), self.s2[f]
            out["min"][f] = float(self.qmin[f]) * Q
            out["max"][f] = float(self.qmax[f]) * Q
            out["mean"][f] = (float(s1) / float(n)) * Q
            if n < 2 ** 33:
                num = n * s2 - s1 * s1
                assert num >= 0
                out["std"][f] = math.sqrt((float(num) / (float(n) * float(n))) * 2.0 ** -40)
        return out

    def stats(self):
        return {k: getattr(self, k) for k in ("observations", "rows_taken", "rows_ignored", "rows_gated", "rows_backfacing")}


def marked(faces, threshold=0.0, sign=0, min_samples=1, min_frames=1, z=0.0):
    n, mean, std = faces["n"], faces["mean"], faces["std"]
    with np.errstate(invalid="ignore"):
        far = np.abs(mean) > threshold if sign == 0 else (mean > threshold if sign > 0 else mean < -threshold)
        m = (n >= min_samples) & (faces["frames"] >= min_frames) & far
        if z > 0:
            m &= np.abs(mean) * np.sqrt(n.astype(np.float64)) > z * std
    return m


class _Columns:
    """What _defect_map_ref.regions reads of a state: its seed is hits > 0 and peak > threshold and frames >= min_frames,
    so the marking goes in as a peak of 1 under the threshold 0.5; `key` is the table's peak column."""

    def __init__(self, faces, mark):
        self.hits = faces["n"]
        self.frames = faces["frames"]
        self.peak = mark.astype(np.float64)
        with np.errstate(invalid="ignore"):
            self.key = np.where(faces["n"] > 0, dref.key_of(np.abs(np.where(faces["n"] > 0, faces["mean"], 0.0))), np.uint64(0))


def regions(model, state, threshold=0.0, sign=0, min_samples=1, min_frames=1, z=0.0, grow=0):
    """_defect_map_ref.regions' dict with measured_area, volume (math.fsum of the rounded products area mean, with
    abs_volume = fsum of their magnitudes for the tests' bound), min_mean, max_mean and n_measured."""
    faces = state.faces()
    mark = marked(faces, threshold, sign, min_samples, min_frames, z)
    out = dref.regions(model, _Columns(faces, mark), threshold=0.5, min_frames=-2 ** 31, grow=grow)
    R = out["n_regions"]
    for k in ("measured_area", "volume", "abs_volume", "min_mean", "max_mean"):
        out[k] = np.full(R, np.nan)
    out["n_measured"] = np.zeros(R, np.int64)
    for r in range(R):
        fs = np.nonzero(out["labels"] == r)[0]
        fs = fs[faces["n"][fs] > 0]
        terms = model.area[fs] * faces["mean"][fs]
        out["n_measured"][r] = len(fs)
        out["measured_area"][r] = math.fsum(model.area[fs])
        out["volume"][r] = math.fsum(terms)
        out["abs_volume"][r] = math.fsum(np.abs(terms))
        if len(fs):
            out["min_mean"][r] = dref.value_of(dref.key_of(faces["mean"][fs]).min(keepdims=True))[0]
            out["max_mean"][r] = dref.value_of(dref.key_of(faces["mean"][fs]).max(keepdims=True))[0]
    return out


def summary(model, state, threshold=0.0, sign=0, min_samples=1, min_frames=1, z=0.0):
    faces = state.faces()
    mark = marked(faces, threshold, sign, min_samples, min_frames, z)
    meas = (faces["n"] > 0) & (faces["n"] >= min_samples)
    a, m = model.area[meas], faces["mean"][meas]
    out = {"faces": model.F, "measured_faces": int(meas.sum()), "marked_faces": int(mark.sum()),
           "total_area": math.fsum(model.area), "measured_area": math.fsum(a), "marked_area": math.fsum(model.area[mark]),
           "s1": math.fsum(a * m), "abs_s1": math.fsum(np.abs(a * m)), "s2": math.fsum(a * (m * m)),
           "max_face": -1, "max_abs_mean": float("nan")}
    if meas.any():
        big = np.abs(m).max()
        out["max_abs_mean"] = float(big)
        out["max_face"] = int(np.nonzero(meas)[0][np.argmax(np.abs(m) == big)])
    return out


# ------------------------------------------------------------------ a clean part under sensor noise
CLEAN = dict(F=1022, per_face=9, sigma=0.5, seed=5, frames=16, z=4.0)     # the seed: see test_deviation_map_cpu.py


def noisy_rows(frame, F=CLEAN["F"], per_face=CLEAN["per_face"], sigma=CLEAN["sigma"], seed=CLEAN["seed"]):
    """One frame of a part without defects: every face measured `per_face` times with N(0, sigma) noise, in face order."""
    rng = np.random.default_rng([seed, frame])
    ids = np.repeat(np.arange(F, dtype=np.uint32), per_face)
    return ids, rng.normal(0.0, sigma, len(ids))
