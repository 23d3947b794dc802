"""The pose rules of include/tri_raster.h ("skeletal poses evaluated on the device") restated in float64 numpy, and the
rigs the animation tests share.

Inputs are the float32 values the float32 implementations see (key times and values, the sample time, the decomposed
per-bone defaults, the inverse bind matrices), promoted exactly; every comparison of times is therefore the same
decision in all three implementations, and only the arithmetic differs. Quaternions are w, x, y, z; matrices are
[16] column-major or [4, 4] indexed [column][row].
"""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)

# E_cpu: the CPU player's worst error against this file over kernel_rigs() x their clips x sample_times(), per matrix
# max |delta entry| / max(1, max |float64 entry|). Measured 2.949e-5 (rig "chain256", clip "slerp", bone 211,
# t = float32(0.2): the rounding of 212 chained float32 products), recorded rounded up to two digits.
# tests/test_animation_cpu.py recomputes it and fails above this value; the device bound is 4 x this constant.
E_CPU = 3.0e-5


# ---- glm restated --------------------------------------------------------------------------------------------------
def qdot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3])


def qnormalize(q):
    q = np.asarray(q, np.float64)
    n = np.sqrt(qdot(q, q))
    if n <= 0.0:
        return np.array([1.0, 0.0, 0.0, 0.0])
    return q * (1.0 / n)


def slerp(a, b, T):
    a, z = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = qdot(a, z)
    if c < 0.0:
        z, c = -z, -c
    if c > 1.0 - FLT_EPSILON:
        return a * (1.0 - T) + z * T
    A = np.arccos(c)
    return (np.sin((1.0 - T) * A) * a + np.sin(T * A) * z) / np.sin(A)


def to_mat3_columns(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)],
                     [2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)],
                     [2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)]])


def quat_cast(cols):
    """glm::quat_cast of the 3x3 matrix with columns cols[0..2]."""
    m = cols
    fx, fy = m[0][0] - m[1][1] - m[2][2], m[1][1] - m[0][0] - m[2][2]
    fz, fw = m[2][2] - m[0][0] - m[1][1], m[0][0] + m[1][1] + m[2][2]
    big, four = 0, fw
    for i, f in ((1, fx), (2, fy), (3, fz)):
        if f > four:
            big, four = i, f
    val = np.sqrt(four + 1.0) * 0.5
    mult = 0.25 / val
    if big == 0:
        return np.array([val, (m[1][2] - m[2][1]) * mult, (m[2][0] - m[0][2]) * mult, (m[0][1] - m[1][0]) * mult])
    if big == 1:
        return np.array([(m[1][2] - m[2][1]) * mult, val, (m[0][1] + m[1][0]) * mult, (m[2][0] + m[0][2]) * mult])
    if big == 2:
        return np.array([(m[2][0] - m[0][2]) * mult, (m[0][1] + m[1][0]) * mult, val, (m[1][2] + m[2][1]) * mult])
    return np.array([(m[0][1] - m[1][0]) * mult, (m[2][0] + m[0][2]) * mult, (m[1][2] + m[2][1]) * mult, val])


def decompose(local_bind):
    """DecomposeBindTransform in float64: (translation, rotation, scale)."""
    m = np.asarray(local_bind, np.float64).reshape(4, 4)
    cols, scale = [], np.zeros(3)
    for j in range(3):
        c = m[j][:3].copy()
        scale[j] = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        cols.append(c / scale[j] if scale[j] > FLT_EPSILON else c)
    return m[3][:3].copy(), qnormalize(quat_cast(cols)), scale


def compose(t, q, s):
    """translate * toMat4(q) * scale as a column-major [16] (q is used as given)."""
    m = np.zeros((4, 4))
    r = to_mat3_columns(np.asarray(q, np.float64))
    for j in range(3):
        m[j][:3] = r[j] * s[j]
    m[3] = [t[0], t[1], t[2], 1.0]
    return m.reshape(16)


# ---- the rules -----------------------------------------------------------------------------------------------------
def _find(times, t):
    """(i, T) for the first i with t < times[i + 1], or None."""
    j = int(np.searchsorted(times[1:], t, side="right"))  # times[1:][j] is the first > t
    if j >= len(times) - 1:
        return None
    a, d32 = float(times[j]), np.float32(times[j + 1]) - np.float32(times[j])
    d = float(times[j + 1]) - a
    T = (float(t) - a) / d if d32 > np.float32(FLT_EPSILON) else 0.0
    return j, min(max(T, 0.0), 1.0)


def sample_vec(track, t, default):
    if track is None or len(track[0]) == 0:
        return default
    times, vals = track
    if len(times) == 1 or t <= times[0]:
        return vals[0].astype(np.float64)
    hit = _find(times, t)
    if hit is None:
        return vals[-1].astype(np.float64)
    i, T = hit
    return vals[i].astype(np.float64) * (1.0 - T) + vals[i + 1].astype(np.float64) * T


def sample_quat(track, t, default):
    if track is None or len(track[0]) == 0:
        return default
    times, vals = track
    if len(times) == 1 or t <= times[0]:
        return qnormalize(vals[0])
    hit = _find(times, t)
    if hit is None:
        return qnormalize(vals[-1])
    i, T = hit
    return qnormalize(slerp(vals[i], vals[i + 1], T))


def traversal(parents, root_index):
    """(order, eval_parent, reached): breadth first from the start set; None when it would never end."""
    n = len(parents)
    if 0 <= root_index < n:
        queue = [root_index]
    else:
        queue = [b for b in range(n) if parents[b] < 0] or [0]
    seen, eval_parent = set(queue), {b: -1 for b in queue}
    q = 0
    while q < len(queue):
        b = queue[q]
        q += 1
        for c in range(n):
            if parents[c] == b:
                if c in seen:
                    return None
                seen.add(c)
                eval_parent[c] = b
                queue.append(c)
    return queue, eval_parent, seen


class Rig:
    """A skeleton as flat arrays: parents, float32 local bind and inverse bind matrices [n, 16], the root index."""

    def __init__(self, name, parents, local_binds, inverse_binds, root_index=-1, source_names=None):
        self.name = name
        self.parents = [int(p) for p in parents]
        self.local_binds = np.ascontiguousarray(local_binds, np.float32).reshape(-1, 16)
        self.inverse_binds = np.ascontiguousarray(inverse_binds, np.float32).reshape(-1, 16)
        self.root_index = root_index
        self.source_names = source_names
        self.clips = []

    @property
    def bones(self):
        return len(self.parents)


class Clip:
    """channels: dicts {bone, T, R, S}, a track being (float32 times [k], float32 values [k, 3 or 4]) or None."""

    def __init__(self, name, duration, channels):
        self.name, self.duration, self.channels = name, float(duration), channels

    def flat(self):
        """(channel rows (bone, T first, T count, R first, R count, S first, S count), vec times/values, quat ...)."""
        rows, vt, vv, qt, qv = [], [], [], [], []
        nv = nq = 0
        for ch in self.channels:
            row = [ch["bone"]]
            for key in ("T", "R", "S"):
                tr = ch.get(key)
                k = 0 if tr is None else len(tr[0])
                if key == "R":
                    row += [nq if k else 0, k]
                    if k:
                        qt.append(tr[0]); qv.append(tr[1]); nq += k
                else:
                    row += [nv if k else 0, k]
                    if k:
                        vt.append(tr[0]); vv.append(tr[1]); nv += k
            rows.append(row)
        cat = lambda parts, shape: (np.concatenate(parts) if parts else np.zeros(shape, np.float32)).astype(np.float32)  # noqa: E731
        return (np.array(rows, np.int64).reshape(-1, 7), cat(vt, (0,)), cat(vv, (0, 3)).reshape(-1, 3), cat(qt, (0,)),
                cat(qv, (0, 4)).reshape(-1, 4))


def evaluate(rig, clip, t, defaults, channel_bones=None):
    """The pose in float64, [bones, 16]. defaults: per bone (translation, rotation, scale) as the float32 host
    decomposition gives them; channel_bones: the resolved bone per channel (default: each channel's own; -1 skips)."""
    n = rig.bones
    t = np.float32(t)
    T = [np.asarray(d[0], np.float64) for d in defaults]
    R = [np.asarray(d[1], np.float64) for d in defaults]
    S = [np.asarray(d[2], np.float64) for d in defaults]
    if clip is not None:
        for c, ch in enumerate(clip.channels):
            b = ch["bone"] if channel_bones is None else int(channel_bones[c])
            if b < 0 or b >= n:
                continue
            T[b] = sample_vec(ch.get("T"), t, T[b])
            R[b] = sample_quat(ch.get("R"), t, R[b])
            S[b] = sample_vec(ch.get("S"), t, S[b])
    local = [compose(T[b], qnormalize(R[b]), S[b]).reshape(4, 4) for b in range(n)]
    walk = traversal(rig.parents, rig.root_index)
    if walk is None:
        return None
    order, eval_parent, reached = walk
    glob = [None] * n
    for b in order:  # [column][row] storage: (P * L) as arrays is L @ P
        glob[b] = local[b] if eval_parent[b] < 0 else local[b] @ glob[eval_parent[b]]
    ident = np.eye(4)
    out = np.zeros((n, 16))
    for b in range(n):
        g = glob[b] if b in reached else local[b]
        if np.array_equal(g, ident):
            g = local[b]
        out[b] = (rig.inverse_binds[b].astype(np.float64).reshape(4, 4) @ g).reshape(16)
    return out


def pose_error(got, ref):
    """The metric of E_cpu: the worst matrix's max |delta| / max(1, max |ref|)."""
    got, ref = np.asarray(got, np.float64).reshape(-1, 16), np.asarray(ref, np.float64).reshape(-1, 16)
    scale = np.maximum(1.0, np.abs(ref).max(axis=1))
    return float((np.abs(got - ref).max(axis=1) / scale).max())


# ---- the shared rigs -----------------------------------------------------------------------------------------------
def _rand_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _bind(rng, reach=0.25, scale_spread=0.02):
    """A local bind transform: a random rotation, a scale near 1, a short translation (chains stay bounded)."""
    s = 1.0 + rng.uniform(-scale_spread, scale_spread, 3)
    return compose(rng.uniform(-reach, reach, 3), _rand_quat(rng), s).astype(np.float32)


def _inverse_binds(parents, local_binds):
    """The inverse of each bone's bind global, in float64, rounded to float32 (what a loader would store)."""
    n = len(parents)
    out = []
    for b in range(n):
        g, seen, p = local_binds[b].astype(np.float64).reshape(4, 4), {b}, parents[b]
        while p >= 0 and p not in seen:  # (a parent loop ends the walk: such bones are test rigs' only)
            seen.add(p)
            g = g @ local_binds[p].astype(np.float64).reshape(4, 4)
            p = parents[p]
        out.append(np.linalg.inv(g).reshape(16))
    return np.stack(out).astype(np.float32)


KEY_COUNTS = (1, 2, 3, 64, 1000)
ROT_SPAN = (0.375, 0.625)  # the rotation tracks of a "hold" clip have all their keys in here


def _times(rng, k, lo, hi):
    """k non-decreasing float32 times in [lo, hi] with duplicates (a zero-length interval) once k >= 3."""
    t = np.sort(rng.uniform(lo, hi, k)).astype(np.float32)
    t[0], t[-1] = lo, hi
    if k >= 3:
        t[k // 2] = t[k // 2 - 1]
    return t


def _quat_keys(rng, k):
    v = np.stack([_rand_quat(rng) for _ in range(k)])
    for i in range(1, k):
        # keep |dot| away from 0 so that float32 and float64 agree on the sign they branch on
        while abs(float(np.dot(v[i - 1], v[i]))) < 0.05:
            v[i] = _rand_quat(rng)
    if k >= 2:
        if np.dot(v[0], v[1]) > 0:
            v[1] = -v[1]  # an obtuse pair: the second is negated
    if k >= 3:
        v[2] = v[1] + np.array([3e-8, -2e-8, 1e-8, 0.0])  # closer than 1e-7: the linear branch
    v = v.astype(np.float32)
    if k >= 64:
        v[k - 2] = 0.0  # a zero-length key inside the track
    return v * np.float32(1.0 + 0.25 * rng.uniform())  # not unit: normalize() has work to do


def _clip(rng, rig, name, rot_span, bones):
    channels = []
    for i, b in enumerate(bones):
        kt, kr, ks = (KEY_COUNTS[(i + j) % len(KEY_COUNTS)] for j in (0, 2, 3))
        if rig.bones > 64 and i % 16:  # big rigs: long tracks on every 16th channel only
            kt, kr, ks = min(kt, 3), min(kr, 3), min(ks, 3)
        ch = {"bone": b,
              "T": (_times(rng, kt, 0.0, 1.0), rng.uniform(-0.3, 0.3, (kt, 3)).astype(np.float32)),
              "R": (_times(rng, kr, *rot_span), _quat_keys(rng, kr)),
              "S": (_times(rng, ks, 0.0, 1.0), (1.0 + rng.uniform(-0.02, 0.02, (ks, 3))).astype(np.float32))}
        if i % 7 == 3:
            ch["S"] = None  # a track without keys leaves the default
        channels.append(ch)
    # one bone with two channels: the later one's tracks win, a track it lacks falls through to the earlier one
    if bones:
        channels.append({"bone": bones[0], "T": (np.array([0.5], np.float32), np.array([[0.1, 0.2, 0.3]], np.float32)),
                         "R": None, "S": None})
    return Clip(name, 1.0, channels)


def make_rig(name, parents, seed, root_index=-1):
    """A rig over `parents` with seeded random bind transforms, matching inverse binds and the "hold" and "slerp" clips."""
    rng = np.random.default_rng(seed)
    lb = np.stack([_bind(rng) for _ in parents])
    rig = Rig(name, parents, lb, _inverse_binds(parents, lb), root_index)
    bones = list(range(rig.bones))
    rig.clips = [_clip(rng, rig, "hold", ROT_SPAN, bones), _clip(rng, rig, "slerp", (0.0, 1.0), bones)]
    return rig


def identity_pair_rig():
    """A parent and a child whose global product is exactly the identity (the child then takes its local)."""
    lb = np.stack([compose([1.0, 2.0, 3.0], [1, 0, 0, 0], [1, 1, 1]), compose([-1.0, -2.0, -3.0], [1, 0, 0, 0], [1, 1, 1])])
    ib = np.stack([compose([0.5, 0.0, 0.0], [1, 0, 0, 0], [1, 1, 1]), compose([0.0, 0.25, 0.0], [1, 0, 0, 0], [2, 2, 2])])
    rig = Rig("identity_pair", [-1, 0], lb, ib, 0)
    rig.clips = []
    return rig


_RIGS = None


def kernel_rigs():
    """The rigs every pose test shares (built once): sizes at which the kernel can still go wrong."""
    global _RIGS
    if _RIGS is None:
        _RIGS = [
            make_rig("one", [-1], 1),
            make_rig("chain3", [-1, 0, 1], 2),
            make_rig("chain128", [-1] + list(range(127)), 3),
            make_rig("chain256", [-1] + list(range(255)), 4),  # every level a barrier; the slice clamps at 128
            make_rig("star128", [-1] + [0] * 127, 5),
            make_rig("forest", [-1, 0, 0, -1, 3, 4], 6, root_index=0),  # bones 3..5 are never reached
            make_rig("forest_noroot", [-1, 0, 0, -1, 3, 4], 7, root_index=-1),  # both roots start
            make_rig("allparented", [2, 0, 2, 1], 8, root_index=-1),  # no parentless bone: bone 0 starts; 2 is its own parent
            identity_pair_rig(),
        ]
    return _RIGS


def sample_times(rig, clip, exact_only):
    """Sample times for a clip: before the first key, after the last, at keys, one ulp either side, inside a
    zero-length interval. exact_only: none strictly inside the rotation span (rotations come from single keys or end
    points, so no sin / acos is evaluated)."""
    f = np.float32
    ts = {f(-0.5), f(0.0), f(1.0), f(1.5), f(ROT_SPAN[0]), f(ROT_SPAN[1])}
    for ch in clip.channels[:3]:
        for key in ("T", "S", "R"):
            tr = ch.get(key)
            if tr is None:
                continue
            for k in {0, len(tr[0]) // 2, len(tr[0]) - 1}:
                t = tr[0][k]
                ts |= {t, np.nextafter(t, f(-np.inf)), np.nextafter(t, f(np.inf))}
    ts |= {f(0.2), f(0.8), np.nextafter(f(0.5), f(0.0)), f(0.5)}
    lo, hi = f(ROT_SPAN[0]), f(ROT_SPAN[1])
    out = sorted(float(t) for t in ts if not (exact_only and lo < t < hi))
    return out
