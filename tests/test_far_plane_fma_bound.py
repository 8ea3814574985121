"""The arithmetic claim behind the one-FMA far planes of the default hot loop (csrc/rt_fastdiv.hpp: CERTIFIED FAR PLANES, ONE FMA EACH),
restated on the CPU in IEEE float32.  Per ray and axis r = RN(1/d) and c = RN(-o * r); per far plane t' = RN(f * r + c) — one rounding, emulated here
exactly (the product of two floats is exact in float64, the sum is taken with its error term and rounded to odd, so the cast to float32 rounds once);
the reference's q = RN(RN(f - o) / d).  With S = max3 |c| and u = 2^-24 the header proves |min3 t' - min3 q| <= 4.01 u |min3 t'| + 1.01 u S and certifies
a box with  |min3 t' - tmin| - 10.5 u |min3 t'| > RN(S * 2.625 u)  and  not 0 <= min3 t' <= RN(S * 2.625 u)  (t' and q have the same sign and are zero together
unless f == o, where q = 0 and t' is a rounding error of at most u S).  Whenever that holds, `tmin <= tmax` and `tmax > 0` taken with t' must be the decisions
taken with q: on uniform rays, on near-axis-parallel rays that start far from the planes (|o / d| up to 2^20 |t|), with tmin within
16 ulp of the far parameter, with planes equal to the origin component (q = 0, t' = a rounding error of either sign), for both signs of d."""
import numpy as np

F = np.float32
U = 2.0 ** -24
EPS_FMA = F(10.5 * U)      # RT_FAR_EPS_FMA
ABS_EPS = F(2.625 * U)     # RT_FAR_ABS_EPS
EPS_PRODUCT = F(8.0 * U)   # RT_FAR_EPS


def fma32(a, b, c):
    """RN(a * b + c) of float32 arrays, one rounding"""
    p = a.astype(np.float64) * b.astype(np.float64)            # exact: 48 bits
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                              # TwoSum: s + e == p + c exactly
    toward = np.where(e > 0, np.inf, -np.inf)
    odd = (s.view(np.int64) & 1) == 1
    s_odd = np.where((e == 0) | odd, s, np.nextafter(s, toward))
    return s_odd.astype(F)


def test_the_fma_emulation_rounds_once():
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is a tie of float32; with c = +-2^-60 the float64 sum lands on that tie, and a second rounding would go to even
    a = np.array([1.0 + 2.0 ** -12], F)
    lo, hi = F(1.0 + 2.0 ** -11), F(1.0 + 2.0 ** -11 + 2.0 ** -23)
    assert fma32(a, a, np.array([0.0], F))[0] == lo                  # the tie itself goes to even,
    assert fma32(a, a, np.array([2.0 ** -60], F))[0] == hi           # a hair more goes up,
    assert fma32(a, a, np.array([-(2.0 ** -60)], F))[0] == lo        # a hair less goes down
    assert F(np.float64(a[0]) * np.float64(a[0]) + 2.0 ** -60) == lo  # (what float64 arithmetic alone would have made of the second case)


def _step_ulps(x, k):
    """x moved by k float32 ulp (k an integer array, either sign)"""
    x = x.copy()
    up = np.where(k > 0, F(np.inf), F(-np.inf)).astype(F)
    k = np.abs(k)
    for _ in range(int(k.max(initial=0))):
        m = k > 0
        x[m] = np.nextafter(x[m], up[m])
        k = k - m
    return x


def _forms(o, d, f):
    """(min3 t', S, min3 of the product form, min3 q) of (m, 3) origins, directions and far planes"""
    r = F(1.0) / d
    c = -(o * r)
    t = fma32(f, r, c)
    prod = (f - o) * r
    q = (f - o) / d
    assert np.all(np.isfinite(t)) and np.all(np.isfinite(q))
    return t.min(axis=1), np.abs(c).max(axis=1), prod.min(axis=1), q.min(axis=1)


def _certain_fma(far, S, tmin):
    """NOT far_pair_uncertain_fma, for one box: the gap less its relative margin, clamped to [0, 1], and the far parameter itself are compared with the per-ray
    term AS UNSIGNED INTEGERS — a far parameter with its sign bit set is the largest of all, so only 0 <= far' <= s_eps raises the question of the sign"""
    gap = np.clip(fma32(np.full_like(far, -EPS_FMA), np.abs(far), np.abs(far - tmin)), F(0), F(1)) + F(0)
    s_eps = (S * ABS_EPS).astype(F)
    return np.minimum(gap.view(np.uint32), far.view(np.uint32)) > s_eps.view(np.uint32)


def _certain_product(far, tmin):
    return np.abs(far - tmin) > np.abs(far) * EPS_PRODUCT


def _rays_and_planes(rng, m, spread=15.0):
    """rays like the probes' (origins within +-spread, Gaussian directions) and, per axis, the plane a ray leaves a random box through"""
    o = ((rng.random((m, 3)) * 2 - 1) * spread).astype(F)
    d = rng.standard_normal((m, 3)).astype(F)
    d[np.abs(d) < 2.0 ** -40] = F(1.0)
    lo = ((rng.random((m, 3)) * 2 - 1) * 12).astype(F)
    hi = (lo + rng.random((m, 3)).astype(F) * F(3) + F(0.01)).astype(F)
    return o, d, np.where(d > 0, hi, lo).astype(F)


def _check(far, S, far_q, tmin):
    certain = _certain_fma(far, S, tmin)
    assert np.array_equal((tmin <= far)[certain], (tmin <= far_q)[certain]), "a certified `tmin <= tmax` differs from the exact one"
    assert np.array_equal((far > 0)[certain], (far_q > 0)[certain]), "a certified `tmax > 0` differs from the exact one"
    return certain


def test_the_proven_bound_holds():
    rng = np.random.default_rng(41)
    o, d, f = _rays_and_planes(rng, 1 << 20)
    d[: 1 << 18] *= np.exp2(-rng.integers(0, 21, (1 << 18, 3))).astype(F)     # near-axis-parallel
    far, S, _, far_q = _forms(o, d, f)
    err = np.abs(far.astype(np.float64) - far_q.astype(np.float64))
    assert np.all(err <= 4.01 * U * np.abs(far.astype(np.float64)) + 1.01 * U * S.astype(np.float64))
    assert (err > 4.01 * U * np.abs(far.astype(np.float64))).any()           # the per-ray term is needed: the relative one alone does not hold


def test_signs_agree_unless_the_plane_is_the_origin_component():
    """per axis: t' and q have the same sign and are zero together when f != o — planes one to three ulp from the origin component included, and origins that
    are powers of two, where the plane below is half an ulp away; with f == o, q is zero and t' a rounding error of o * r, at most u |c|, of either sign"""
    rng = np.random.default_rng(45)
    m = 1 << 20
    o, d, f = _rays_and_planes(rng, m)
    o, d, f = o.reshape(-1), d.reshape(-1), f.reshape(-1)
    pow2 = rng.random(3 * m) < 0.1
    o[pow2] = (np.exp2(rng.integers(-10, 5, int(pow2.sum()))) * np.where(rng.random(int(pow2.sum())) < 0.5, -1, 1)).astype(F)
    o[rng.random(3 * m) < 0.02] = F(0)
    close = (rng.random(3 * m) < 0.6) & (o != 0)          # (a plane a few ulp from zero is a denormal: outside the class)
    f = np.where(close, _step_ulps(o, rng.integers(-3, 4, 3 * m)), f).astype(F)
    r = F(1.0) / d
    c = -(o * r)
    t, q = fma32(f, r, c), (f - o) / d
    same = f == o
    assert same.mean() > 0.05 and (~same & close).mean() > 0.4
    assert np.array_equal(np.sign(t)[~same], np.sign(q)[~same]) and not (t[~same] == 0).any()
    assert not q[same].any() and np.all(np.abs(t[same]) <= U * np.abs(c[same]).astype(np.float64) * 1.01)
    assert (t[same] > 0).any() and (t[same] < 0).any()


def test_uniform_rays_certify_and_decide_exactly():
    rng = np.random.default_rng(42)
    m = 1 << 20
    o, d, f = _rays_and_planes(rng, m)
    assert (d < 0).mean() > 0.4 and (d > 0).mean() > 0.4                     # both signs of d
    far, S, far_p, far_q = _forms(o, d, f)
    tmin = (far_q * rng.uniform(-2, 3, m)).astype(F)
    certain = _check(far, S, far_q, tmin)
    unsure, unsure_p = 1.0 - certain.mean(), 1.0 - _certain_product(far_p, tmin).mean()
    print(f"uniform regular cases: uncertain {unsure:.2e} (fma form), {unsure_p:.2e} (product form)")
    assert unsure < 1e-3       # a margin that certifies nothing would be sound and useless
    assert unsure_p < 1e-3     # the generator is fair: the present certificate stays under the same cap


def test_adversarial_families_never_certify_a_wrong_decision():
    rng = np.random.default_rng(43)
    m = 1 << 20
    o, d, f = _rays_and_planes(rng, m)
    fam = np.arange(m) % 4
    # family 1: near-axis-parallel rays that start far from the planes — one or two direction components scaled down by up to 2^20, so |o / d| ~ 2^20 |t|
    k1 = fam == 1
    small = rng.random((m, 3)) < 0.5
    small[np.arange(m), rng.integers(0, 3, m)] = False                       # at least one component stays
    scale = np.exp2(-rng.integers(1, 21, (m, 3))).astype(F)
    d[k1] = np.where(small[k1], d[k1] * scale[k1], d[k1])
    o[k1] = (o[k1] * np.exp2(rng.integers(0, 8, (int(k1.sum()), 1))).astype(F)).astype(F)
    # family 2: a plane equal to the origin component on one or more axes (q = 0 there; t' is the rounding error of o * r)
    k2 = fam == 2
    same = rng.random((m, 3)) < 0.4
    same[np.arange(m), rng.integers(0, 3, m)] = True
    f = np.where(k2[:, None] & same, o, f).astype(F)
    # family 3: both at once, and origins within a few ulp of a plane
    k3 = fam == 3
    d[k3] = np.where(small[k3], d[k3] * scale[k3], d[k3])
    near = _step_ulps(o.reshape(-1), rng.integers(-3, 4, 3 * m)).reshape(m, 3)
    f = np.where(k3[:, None] & same, near, f).astype(F)
    far, S, _, far_q = _forms(o, d, f)
    assert (S[k1] > 2.0 ** 18 * np.abs(far[k1])).mean() > 0.02               # the family reaches |o / d| >> |t|
    # tmin: half within 0 .. 16 ulp of the far parameter (either side, of the exact and of the fma form), a quarter exactly zero or -+ tiny, the rest random
    tmin = (far_q * rng.uniform(-2, 3, m)).astype(F)
    h = m // 2
    tmin[:h] = _step_ulps(np.where(rng.random(h) < 0.5, far_q[:h], far[:h]).astype(F), rng.integers(-16, 17, h))
    z = slice(h, h + m // 4)
    tmin[z] = np.where(rng.random(m // 4) < 0.5, F(0.0), (rng.standard_normal(m // 4) * 1e-6).astype(F))
    certain = _check(far, S, far_q, tmin)
    # the set really holds decisions the fma form gets wrong, all of them refused; and the certificate is not vacuous on it
    wrong = ((tmin <= far) != (tmin <= far_q)) | ((far > 0) != (far_q > 0))
    sign_wrong = (far > 0) != (far_q > 0)
    print(f"adversarial cases: certain {certain.mean():.3f}, wrong with the fma form {wrong.sum()} (sign {sign_wrong.sum()}), certified wrong {(wrong & certain).sum()}")
    assert wrong.sum() > 1000 and sign_wrong.sum() > 100 and not (wrong & certain).any()
    assert 0.1 < certain.mean() < 0.9
