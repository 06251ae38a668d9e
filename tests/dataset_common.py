"""Yardstick of the dataset-builder tests: a numpy restatement of the reference's clip-image chain with the reference's
precision at every stage (float32 through canonicalisation, contact labels and floor shift; float64 from the reference joint
on), the seeded inputs shared by tests/golden/make_dataset.py and the tests, and the gates.

TEST INFRASTRUCTURE ONLY.  The restatement is first held to the reference's own output (tests/golden/dataset_repr*.npz,
written by make_dataset.py from loader/train_loader_infill.py / train_loader_smooth.py): images to 1e-12, labels and
statistics exactly; only then is it used at the shapes the fixture does not cover.
"""
import os

import numpy as np

from oracle import markers_oracle as MO

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
FOOT = (16, 47, 30, 60)
F32 = np.float32
EPS32 = 2.0 ** -24                       # one fp32 rounding, relative


def load_fixture():
    out = {}
    for name in ('dataset_repr.npz', 'dataset_repr_inputs.npz', 'dataset_repr_smooth.npz'):      # three files: 1 MiB each at most
        with np.load(os.path.join(GOLDEN, name)) as z:
            out.update({k: z[k] for k in z.files})
    return out


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------
def _smooth(rng, T, n, scale, width=6.0):
    x = rng.standard_normal((T + 48, n))
    k = np.exp(-0.5 * (np.arange(-24, 25) / width) ** 2)
    x = np.stack([np.convolve(x[:, i], k / k.sum(), 'valid') for i in range(n)], 1)[:T]
    return x * scale


def synthetic_clips(seed, n, T, still=True):
    """AMASS-shaped clips (what ``divide_clip`` leaves in ``data_dict_list``): the body stands almost still for the first
    third (so that some feet are in contact) and walks off afterwards.  Values are float32-representable float64, like a
    file whose numbers went through ``.float()``."""
    rng = np.random.default_rng(seed)
    clips = []
    for i in range(n):
        ramp = np.clip((np.arange(T) - T / 3.0) / (T / 3.0), 0.0, 1.0)[:, None] if still else np.ones((T, 1))
        poses = _smooth(rng, T, 156, 0.6) * (0.02 + ramp) + rng.standard_normal(156) * 0.15
        poses[:, 66:] *= 0.3
        axis = rng.standard_normal(3)
        poses[:, :3] = _smooth(rng, T, 3, 0.5) * (0.02 + ramp) + axis / np.linalg.norm(axis) * rng.uniform(0.0, np.pi)
        vel = _smooth(rng, T, 3, 0.05) * ramp + 1e-4 * rng.standard_normal((T, 3))
        trans = np.cumsum(vel, 0) + rng.standard_normal(3) * [1.0, 1.0, 0.2]
        clips.append(dict(poses=poses.astype(F32).astype(np.float64), trans=trans.astype(F32).astype(np.float64),
                          betas=(rng.standard_normal(16) * 0.8).astype(F32).astype(np.float64),
                          gender='male' if (i + seed) % 2 == 0 else 'female', mocap_framerate=120))
    return clips


def synthetic_markers(seed, n, T, M=67):
    """world-frame markers / pelvis / hips of a plausible moving body without a body model: a marker cloud that turns and
    walks, the direction markers (26 / 56, 27 / 57) left and right of the pelvis, feet near the floor and partly at rest"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-0.3, 0.3, (M, 3)) * [1.0, 0.5, 1.0]
    base[:, 2] = rng.uniform(0.0, 1.6, M)
    for l, r in ((26, 56), (27, 57)):
        base[l, :2], base[r, :2] = [-0.2, 0.02 * l / 27.0], [0.2, -0.01]
    for f in FOOT:
        base[f, 2] = rng.uniform(0.0, 0.05)
    markers, pelvis, hips = [], [], []
    for _ in range(n):
        ramp = np.clip((np.arange(T) - T / 3.0) / max(T / 3.0, 1.0), 0.0, 1.0)
        yaw = rng.uniform(-3, 3) + np.cumsum(_smooth(rng, T, 1, 0.08)[:, 0] * ramp)
        pos = np.cumsum(_smooth(rng, T, 3, 0.04) * ramp[:, None] * [1, 1, 0.05], 0) + rng.standard_normal(3) * [2, 2, 0.1] + [0, 0, 0.9]
        c, s = np.cos(yaw), np.sin(yaw)
        wob = _smooth(rng, T, M * 3, 0.03).reshape(T, M, 3) * ramp[:, None, None]
        loc = base[None] + wob - [0, 0, 0.9]
        x = c[:, None] * loc[..., 0] - s[:, None] * loc[..., 1]
        y = s[:, None] * loc[..., 0] + c[:, None] * loc[..., 1]
        markers.append(np.stack([x, y, loc[..., 2]], -1) + pos[:, None])
        pelvis.append(pos + _smooth(rng, T, 3, 0.01))
        h = np.array([[-0.1, 0.0, -0.05], [0.1, 0.0, -0.05]])
        hips.append(np.stack([c[0] * h[:, 0] - s[0] * h[:, 1], s[0] * h[:, 0] + c[0] * h[:, 1], h[:, 2]], -1) + pos[0])
    return np.asarray(markers, F32), np.asarray(pelvis, F32), np.asarray(hips, F32)


def amass_sequences(seed=11):
    """tiny AMASS-shaped sequences for ``divide_clips``: framerates 60 / 120 / 150 (kept), 100 (skipped), one too short"""
    rng = np.random.default_rng(seed)
    out = []
    for fps, n, gender in ((60, 130, 'male'), (120, 250, 'female'), (150, 160, 'male'), (100, 300, 'female'), (60, 50, 'male'), (120, 120, 'female')):
        out.append(dict(poses=rng.standard_normal((n, 156)), trans=rng.standard_normal((n, 3)), betas=rng.standard_normal(16),
                        dmpls=rng.standard_normal((n, 8)), gender=np.array(gender), mocap_framerate=np.array(float(fps))))
    return out


# ---- the chain -------------------------------------------------------------------------------------------------------------
def canonicalise(markers, pelvis, hips0, smooth=False):
    """float32, one clip: markers [T, M, 3], pelvis [T, 3], hips0 [2, 3] -> (markers, pelvis) in the first frame's frame
    (train_loader_infill.py:136-146; train_loader_smooth.py:142-143 subtracts marker 0 of frame 0 from the markers)"""
    markers, pelvis, hips0 = np.asarray(markers, F32), np.asarray(pelvis, F32), np.asarray(hips0, F32)
    x = hips0[1] - hips0[0]
    x[2] = 0
    x = x / np.sqrt((x * x).sum(dtype=F32))
    z = np.array([0, 0, 1], F32)
    y = np.cross(z, x).astype(F32)
    y = y / np.sqrt((y * y).sum(dtype=F32))
    R = np.stack([x, y, z], 1).astype(F32)
    # out = fma(dy, R[1], fl(dx * R[0])), the kernel's form (the up column of R is (0, 0, 1)); the float64 sum of an exact product
    # and a float32 is the fused result unless it falls on a float32 tie.  NOTE: for this fp32 stage the comparison "kernel against
    # restatement" is therefore a comparison of one formula with itself (it checks indexing, not the choice of roundings); what ties
    # the formula to the reference is the fixture: a{T}_body, the loader's own canonicalised body, within 3 roundings
    # (check_restatement_is_the_reference), and the reference's images under the sens gate (check_kernel_vs_fixture).
    f64 = np.float64
    fma = lambda a, b, c: (a.astype(f64) * f64(b) + c.astype(f64)).astype(F32)
    mul = lambda p: np.stack([fma(p[..., 1], R[1, 0], p[..., 0] * R[0, 0]), fma(p[..., 1], R[1, 1], p[..., 0] * R[0, 1]), p[..., 2]], -1)
    return mul(markers - (markers[0, 0] if smooth else pelvis[0])), mul(pelvis - pelvis[0])


def foot_margins(m, fps=30.0):
    """(speed [T-1, 4], height [T, 4], height threshold) of the foot markers of one canonicalised clip, float32"""
    feet = m[:, list(FOOT)]
    v = (feet[1:] - feet[:-1]) * F32(fps)
    speed = np.sqrt((v * v).sum(-1, dtype=F32))
    return speed, feet[:, :, 2], m[:, :, 2].min() + F32(0.10)


def contact_labels(m, fps=30.0):
    speed, height, thr = foot_margins(m, fps)
    low = (height < thr).astype(F32)
    lbl = np.zeros_like(low)
    lbl[:-1][speed < F32(0.22)] = 1.0
    lbl = lbl * low
    lbl[-1] = low[-1]
    return lbl


def raw_4chan_from_body(body, fps=30.0):
    """canonicalised pelvis + markers [T, 1 + M, 3] float32 -> (image [4, T-1, d] float64, rot_0_pivot, labels [T, 4])"""
    body = np.asarray(body, F32)
    lbl = contact_labels(body[:, 1:], fps)
    shifted = body.copy()
    shifted[:, :, 2] = shifted[:, :, 2] - shifted[:, :, 2].min()               # float32, like cur_body at :220
    img, piv = MO.get_local_markers_4chan(shifted.astype(np.float64), lbl.astype(np.float64))
    return img, piv, lbl


def raw_4chan(markers, pelvis, hips0, fps=30.0):
    """-> (image [4, T-1, d] float64, rot_0_pivot, labels [T, 4], canonicalised pelvis + markers [T, 1 + M, 3] float32)"""
    m, p = canonicalise(markers, pelvis, hips0)
    body = np.concatenate([p[:, None], m], 1)
    return raw_4chan_from_body(body, fps) + (body,)


def raw_smooth(markers, pelvis, hips0):
    """-> image [T, d] float32 (train_loader_smooth.py:169-174)"""
    m, p = canonicalise(markers, pelvis, hips0, smooth=True)
    return np.concatenate([p[:, None], m - p[:, None]], 1).reshape(len(p), -1)


def stats_4chan(imgs):
    """train_loader_infill.py:305-316 on [N, 4, T-1, d] float64"""
    d = imgs.shape[-1]
    Xmean_local = imgs[:, 0].mean(axis=1).mean(axis=0)
    Xmean_local[-4:] = 0.0
    Xstd_local = np.ones(d)
    Xstd_local[0:] = imgs[:, 0].std()
    Xstd_local[-4:] = 1.0
    return dict(Xmean_local=Xmean_local, Xstd_local=Xstd_local, Xmean_global_xy=imgs[:, 1:3].mean(), Xstd_global_xy=imgs[:, 1:3].std(),
                Xmean_global_r=imgs[:, 3].mean(), Xstd_global_r=imgs[:, 3].std())


def stats_smooth(imgs):
    """train_loader_smooth.py:184-197 on [N, T, d] (float32 there: so are its statistics)"""
    Xmean = imgs.mean(axis=1).mean(axis=0)[np.newaxis, np.newaxis, :]
    Xstd = np.ones(imgs.shape[-1]) * imgs.std()
    Xstd[0:3] = imgs[:, :, 0:3].std()
    return dict(Xmean=Xmean, Xstd=Xstd)


def normalise_4chan(imgs, s):
    out = np.array(imgs, np.float64)
    out[:, 0] = (out[:, 0] - s['Xmean_local']) / s['Xstd_local']
    out[:, 1:3] = (out[:, 1:3] - s['Xmean_global_xy']) / s['Xstd_global_xy']
    out[:, 3] = (out[:, 3] - s['Xmean_global_r']) / s['Xstd_global_r']
    return out


def normalise_smooth(imgs, s):
    out = np.array(imgs)
    out[:, :, 0:3] = (out[:, :, 0:3] - s['Xmean'][:, :, 0:3]) / s['Xstd'][0:3]
    return out


def stats_vector(s, d, four):
    """the layout lemo_decode_clip / lemo_clip_repr_write read"""
    v = np.zeros(2 * d + 4)
    if four:
        v[:d], v[d:2 * d] = s['Xmean_local'], s['Xstd_local']
        v[2 * d:] = [s['Xmean_global_xy'], s['Xstd_global_xy'], s['Xmean_global_r'], s['Xstd_global_r']]
    else:
        v[:d], v[d:2 * d] = np.asarray(s['Xmean'], np.float64).reshape(-1), s['Xstd']
        v[2 * d], v[2 * d + 1] = s['Xstd'][3], s['Xstd'][0]
    return v


def stats_f64(raw, four):
    """numpy float64 statistics of unnormalised images ([N, 4, F, d] / [N, F, d]) in that layout: what the native
    statistics pass is held to"""
    raw = np.asarray(raw, np.float64)
    return stats_vector(stats_4chan(raw) if four else stats_smooth(raw), raw.shape[-1], four)


def perturb_ulp(x, rng):
    """every float32 moved by one ulp up or down"""
    x = np.asarray(x, F32)
    return np.nextafter(x, np.where(rng.random(x.shape) < 0.5, -np.inf, np.inf).astype(F32))


def sens_of(fn, args, n=8, seed=99):
    """largest change of ``fn(*args)`` (an array or a tuple of arrays) over ``n`` seeded one-ulp perturbations of the float32
    arguments: the scale the gates are written in"""
    rng = np.random.default_rng(seed)
    tup = lambda r: r if isinstance(r, tuple) else (r,)
    base = tup(fn(*args))
    worst = [0.0] * len(base)
    for _ in range(n):
        got = tup(fn(*[perturb_ulp(a, rng) for a in args]))
        worst = [max(w, float(np.abs(np.asarray(g, np.float64) - np.asarray(b, np.float64)).max())) for w, g, b in zip(worst, got, base)]
    return worst


def gate(sens, ref):
    """4 x sens plus one fp32 rounding of the stored value, elementwise"""
    return 4.0 * sens + EPS32 * np.abs(np.asarray(ref, np.float64)) + 1e-45
