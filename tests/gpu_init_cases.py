"""The seeded scenes of the Initializer tests, shared by the CPU and GPU files (built once; test_initializer_reference.py checks on the CPU that they are what they
claim to be).  KITTI intrinsics; points at 4-20 m depth (general) or on one plane at 8 m (planar); the motion is a 0.3 m baseline with a 0.02 rad yaw; keys are rounded
to float; some keys of each frame are unmatched, so n1, n2 > N and Normalize sees keys the matches do not."""
import functools
import numpy as np
import initializer_reference as R

KITTI = (718.856, 718.856, 607.1928, 185.2157)
WIDTH, HEIGHT = 1241, 376
PARAMS = dict(sigma=1.0, max_iterations=200, min_parallax=1.0, min_triangulated=50)            # Tracking.cc:573 and Initializer.cc:116-118


def motion(yaw=0.02, baseline=0.3):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), np.array([baseline, 0.0, 0.0])


def scene(seed, N, kind="general", noise=0.0, extra=(7, 5), yaw=0.02, baseline=0.3):
    """-> (problem dict(keys1 [n1, 2], keys2 [n2, 2], matches12 [n1], K), truth dict(R, t, X [N, 3] in camera 1 by match, plane (n, d) or None))"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = KITTI
    if kind == "rotation":
        baseline = 0.0
    if kind == "identity":
        yaw = baseline = 0.0
    Rt, tt = motion(yaw, baseline)
    uv1 = np.stack([rng.uniform(20, WIDTH - 20, N), rng.uniform(20, HEIGHT - 20, N)], axis=1)
    ray = np.stack([(uv1[:, 0] - cx) / fx, (uv1[:, 1] - cy) / fy, np.ones(N)], axis=1)
    plane = None
    if kind in ("planar", "identity"):
        n = np.array([0.2, 0.1, 1.0]); n /= np.linalg.norm(n); d = 8.0 * n[2]                 # n . X = d: 8 m on the optical axis
        z = d / (ray @ n); plane = (n, d)
    else:
        z = rng.uniform(4.0, 20.0, N)
    X = ray * z[:, None]
    X2 = X @ Rt.T + tt
    uv2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], axis=1)
    if noise:
        uv1 = uv1 + rng.normal(0, noise, uv1.shape); uv2 = uv2 + rng.normal(0, noise, uv2.shape)
    n1, n2 = N + extra[0], N + extra[1]
    keys1 = np.stack([rng.uniform(0, WIDTH, n1), rng.uniform(0, HEIGHT, n1)], axis=1); keys2 = np.stack([rng.uniform(0, WIDTH, n2), rng.uniform(0, HEIGHT, n2)], axis=1)
    i1 = np.sort(rng.permutation(n1)[:N]); i2 = rng.permutation(n2)[:N]
    keys1[i1] = uv1; keys2[i2] = uv2
    matches12 = np.full(n1, -1, np.int32); matches12[i1] = i2
    pr = dict(keys1=keys1.astype(np.float32), keys2=keys2.astype(np.float32), matches12=matches12, K=KITTI)
    return pr, dict(R=Rt, t=tt, X=X, plane=plane, i1=i1, i2=i2)


def coincident(N, extra=(3, 2)):
    """every key of both frames is one point: Normalize divides by a zero deviation and NaN flows through both RANSACs"""
    n1, n2 = N + extra[0], N + extra[1]
    keys1 = np.full((n1, 2), 100.0, np.float32); keys2 = np.full((n2, 2), 120.0, np.float32)
    matches12 = np.full(n1, -1, np.int32); matches12[:N] = np.arange(N)
    return dict(keys1=keys1, keys2=keys2, matches12=matches12, K=KITTI)


def _case(name, pr, seed, **kw):
    p = dict(PARAMS); p.update(kw)
    return dict(name=name, problem=pr, rand=R.draws(seed, 1, p["max_iterations"])[0], params=p)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case: one problem, its draws and the call's parameters"""
    out = []
    for k, N in enumerate((8, 9, 63, 64, 65, 129, 200)):
        out.append(_case("general%d" % N, scene(100 + k, N, "general", 0.0 if N % 2 else 0.5)[0], 100 + k))
    out.append(_case("general129_one_iteration", scene(105, 129, "general")[0], 7, max_iterations=1))
    out.append(_case("planar65", scene(120, 65, "planar")[0], 120))
    out.append(_case("planar65_ok", scene(210, 65, "planar")[0], 210))
    out.append(_case("planar129_ok", scene(210, 129, "planar")[0], 210))
    out.append(_case("general64_ok", scene(205, 64, "general", 0.5)[0], 205))
    out.append(_case("planar200_noise", scene(121, 200, "planar", 0.5)[0], 121))
    out.append(_case("planar64_one_iteration", scene(122, 64, "planar")[0], 122, max_iterations=1))
    out.append(_case("rotation129", scene(130, 129, "rotation", 0.5)[0], 130))
    out.append(_case("rotation65_exact", scene(131, 65, "rotation")[0], 131))
    out.append(_case("identity64", scene(140, 64, "identity")[0], 140))
    out.append(_case("few40", scene(150, 40, "general")[0], 150))
    tie = _case("tie65", scene(160, 65, "general", 0.5)[0], 160, max_iterations=4)
    tie["rand"] = tie["rand"].copy(); tie["rand"][2] = tie["rand"][0]; tie["rand"][3] = tie["rand"][1]
    out.append(tie)
    out.append(_case("coincident20", coincident(20), 170, max_iterations=3))
    return {c["name"]: c for c in out}


@functools.lru_cache(maxsize=None)
def expected(name):
    """the definition's answer for a case (computed once, not to be modified)"""
    c = cases()[name]; pr = c["problem"]
    return R.initialize(pr["keys1"], pr["keys2"], pr["matches12"], pr["K"], c["rand"], **c["params"])


def batch():
    """three problems of different N, n1 and n2 for one call"""
    names = ("general65", "planar200_noise", "general129")
    return [cases()[n] for n in names]
