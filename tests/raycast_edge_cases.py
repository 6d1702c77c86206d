"""The ray casters' primitives at their edges: independent fp64 statements of the sphere, the capsule and the box, and the builders of the crafted
scenes that tests/test_raycast_edge_cases.py (CPU: are the cases what they claim to be?) and tests/test_gpu_raycast_edges.py (GPU: do the three
libraries see them?) share.  Pure numpy: no torch, no GPU, no other test module.

Every scene is cast from ORIGIN by a sensor at identity pose: the env's base stands at ORIGIN with the identity quaternion, the depth camera and
the LiDAR are mounted at the torso's origin, the renderer's fixed camera sits there too (azimuth 0, elevation 0).  The floor is then 4 m below:
beyond FAR for the two sensors on every ray; the renderer, which has no `far`, sees it below the horizon, and expected() makes it part of the
expectation.  A geom's position is a multiple of GRID, so that ORIGIN + pos - ORIGIN is exact in fp32 and the libraries place the primitive where
the reference does; quaternions, radii and half lengths are rounded to fp32 first and the reference is handed those rounded values
(realise_geom).  A rounded quaternion moves a 1e-6 rad tilt, so a capsule case records the angle and the lateral distance actually realised."""
import numpy as np

W, H, FOVY = 9, 7, 60.0                                   # odd on purpose: the centre column has u = 0 and the centre row v = 0, exactly
NEAR, FAR = 0.01, 3.0
ORIGIN = np.array([0.0, 0.0, 4.0])
GRID = 2.0 ** -20
MARGIN = 1e-3                                             # metres (slabs, origins) or relative (ties, far): what "unambiguous" means below
SPHERE, CAPSULE, BOX = 0, 1, 2                            # render.SPHERE ...
SEG_SKY, SEG_PLANE, SEG_BOX, SEG_GEOM = -1, 0, 1, 1000    # render.SEG_...
MAX_GEOM = 32

ANGLES = (0.0, 1e-6, 1e-5, 1e-4, 3e-4, 1e-3, 1e-2, 0.3)   # rad between the ray and the capsule's axis
OFFSETS = (0.0, 0.5, 0.9, 1.1)                            # lateral distance of the ray from the axis in radii: three hits, one miss
# 0.9 r and 1.1 r, pulled to the safe side by one part in 1e4: the fp32 rounding of the inputs (some 1e-6 m at 2.5 m against radii of 0.013 m
# and more) must not put a realised case on the wrong side of the bounds "hit <= 0.9 r" and "miss >= 1.1 r" that the CPU test asserts
K_REALISED = {0.0: 0.0, 0.5: 0.5, 0.9: 0.9 * (1 - 1e-4), 1.1: 1.1 * (1 + 1e-4)}
DISTANCES = (0.3, 2.5)                                    # origin to the capsule's centre
GOLDEN = np.pi * (3.0 - np.sqrt(5.0))
GREY = np.array([0.5, 0.5, 0.5])


def f32(x):
    """x rounded to fp32, as float64"""
    return np.asarray(x, np.float32).astype(np.float64)


def unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


def qmat(q):
    """rotation matrix of the normalised quaternion wxyz: columns = the frame's axes"""
    w, x, y, z = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def quat_z_to(u):
    """unit quaternion wxyz that turns +z onto the unit vector u"""
    c = float(u[2])
    if c < -1.0 + 1e-12:
        return np.array([0.0, 1.0, 0.0, 0.0])
    q = np.array([1.0 + c, -u[1], u[0], 0.0])
    return q / np.linalg.norm(q)


def perpendiculars(d):
    """two unit vectors perpendicular to the unit vector d and to each other"""
    helper = np.array([0.0, 0.0, 1.0]) if abs(d[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    p = unit(np.cross(d, helper))
    return p, np.cross(d, p)


# ---------------------------------------------------------------- the primitives (ray o + t d, o [3], d [P, 3] unit rows; a hit needs t > 0)
def hit_plane(o, d):
    t = np.full(len(d), np.inf)
    m = d[:, 2] != 0
    t[m] = -o[2] / d[m, 2]
    return np.where(t > 0, t, np.inf)


def hit_sphere(o, d, c, r):
    """closed form: with m = the foot of the centre on the ray, the entry lies sqrt(r^2 - |centre - m|^2) before m.  A sphere that holds the
    origin, or lies behind it, is not seen.  (o may also be [P, 3]: an origin per ray)"""
    oc = np.asarray(c, float) - o
    along = np.sum(d * oc, -1)
    lat2 = np.sum(np.cross(d, oc) ** 2, -1)
    half = np.sqrt(np.maximum(r * r - lat2, 0.0))
    t = along - half
    return np.where((lat2 <= r * r) & (t > 0), t, np.inf)


def hit_capsule(o, d, c, ax, r, hl):
    """The capsule as the union of three convex pieces, the origin outside all of them: the cylinder of radius r about the segment c +- hl ax, and
    the two end spheres.  The first hit of the union is the smallest of the three entries.  The cylinder in the projected form: with
    d_perp = d - (d.ax) ax and o_perp likewise, solve |o_perp + t d_perp| = r and take the entry when |d_perp|^2 > 0, t > 0 and the axial
    coordinate s of the entry point has |s| < hl.  (An entry through a flat end lies inside that end's sphere, which is entered earlier.)
    (o may also be [P, 3]: an origin per ray)"""
    ax = unit(ax)
    oc = o - np.asarray(c, float)
    s_o, s_d = oc @ ax, d @ ax
    o_perp, d_perp = oc - np.asarray(s_o)[..., None] * ax, d - s_d[:, None] * ax[None]
    A, B, C = np.sum(d_perp * d_perp, -1), np.sum(d_perp * o_perp, -1), np.sum(o_perp * o_perp, -1) - r * r
    disc = B * B - A * C
    ok = (A > 0) & (disc >= 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ok, (-B - np.sqrt(np.where(ok, disc, 0.0))) / np.where(ok, A, 1.0), np.inf)
        s = s_o + t * s_d
    cyl = np.where(ok & (t > 0) & (np.abs(s) < hl), t, np.inf)
    return np.minimum(cyl, np.minimum(hit_sphere(o, d, c - hl * ax, r), hit_sphere(o, d, c + hl * ax, r)))


def hit_box(o, d, c, A, h, axis=False):
    """Slab test in the box frame (A: columns = the box's axes, h: half extents): the entry distance; a ray that starts inside does not see the box.
    A direction component that is exactly 0 along an axis: with |ol| < h that axis is no constraint, with |ol| > h the ray misses.
    axis=True: -> (t, the axis of the entry face)"""
    ol, dl = (o - np.asarray(c, float)) @ A, d @ A
    tn, tf = np.full(len(d), -np.inf), np.full(len(d), np.inf)
    face = np.zeros(len(d), int)
    miss = np.zeros(len(d), bool)
    for k in range(3):
        zero = dl[:, k] == 0
        miss |= zero & (abs(ol[k]) > h[k])
        inv = 1.0 / np.where(zero, 1.0, dl[:, k])
        t1, t2 = (-h[k] - ol[k]) * inv, (h[k] - ol[k]) * inv
        lo, hi = np.where(zero, -np.inf, np.minimum(t1, t2)), np.where(zero, np.inf, np.maximum(t1, t2))
        face = np.where(lo > tn, k, face)
        tn, tf = np.maximum(tn, lo), np.minimum(tf, hi)
    t = np.where(~miss & (tn <= tf) & (tn > 0), tn, np.inf)
    return (t, face) if axis else t


def hit_prim(o, d, p):
    if p["type"] == SPHERE:
        return hit_sphere(o, d, p["c"], p["r"])
    if p["type"] == CAPSULE:
        return hit_capsule(o, d, p["c"], p["ax"], p["r"], p["hl"])
    return hit_box(o, d, p["c"], p["A"], p["h"])


# ---------------------------------------------------------------- what the libraries are given -> what the reference is given
def geom(kind, pos, quat, size):
    """a robot primitive on the torso in the form of render.default_robot_geoms, every number representable: pos on GRID, the rest fp32"""
    pos = np.round(np.asarray(pos, float) / GRID) * GRID
    assert np.array_equal(f32(pos), pos) and np.array_equal(f32(ORIGIN + pos), ORIGIN + pos)
    return dict(body=0, type=kind, pos=pos, quat=f32(quat), size=f32(list(size) + [0.0] * (3 - len(size))), rgb=GREY)


def realise_geom(g):
    """the primitive that a geom dict describes with the base at ORIGIN, identity orientation"""
    c, R = ORIGIN + g["pos"], qmat(g["quat"])
    if g["type"] == SPHERE:
        return dict(type=SPHERE, c=c, r=g["size"][0])
    if g["type"] == CAPSULE:
        return dict(type=CAPSULE, c=c, ax=R[:, 2], r=g["size"][0], hl=g["size"][1])
    return dict(type=BOX, c=c, A=R, h=g["size"].copy())


def terrain_table(rows):
    """[[centre, half extents], ...] of boxes aligned with the world axes -> the [1, B, 10] float32 table the libraries take"""
    tab = np.zeros((1, len(rows), 10), np.float32)
    for b, (c, h) in enumerate(rows):
        tab[0, b, 0:3], tab[0, b, 3], tab[0, b, 7:10] = c, 1.0, h
    return tab


def realise_terrain(tab):
    return [dict(type=BOX, c=r[0:3].astype(float), A=qmat(r[3:7].astype(float)), h=r[7:10].astype(float)) for r in tab[0]]


def scene_prims(scene):
    """-> (the primitives of a scene in the libraries' order: boxes, then geoms; their segmentation ids)"""
    boxes = realise_terrain(scene["terrain"]) if scene.get("terrain") is not None else []
    geoms = [realise_geom(g) for g in scene["geoms"]]
    return boxes + geoms, [SEG_BOX + b for b in range(len(boxes))] + [SEG_GEOM + g for g in range(len(geoms))]


def expected(scene, dirs, plane=True):
    """The fp64 cast of a scene along all of a sensor's rays; nothing is culled.  -> dict(t [R] distance along the ray (inf: nothing),
    seg [R], second [R] the next candidate's distance, T [R, 1 + n] every candidate: the plane first)"""
    prims, ids = scene_prims(scene)
    T = np.stack([hit_plane(ORIGIN, dirs) if plane else np.full(len(dirs), np.inf)] + [hit_prim(ORIGIN, dirs, p) for p in prims], 1)
    order = np.argsort(T, 1, kind="stable")
    t = np.take_along_axis(T, order[:, :1], 1)[:, 0]
    second = np.take_along_axis(T, order[:, 1:2], 1)[:, 0] if T.shape[1] > 1 else np.full(len(t), np.inf)
    seg = np.where(np.isfinite(t), np.array([SEG_PLANE] + ids)[order[:, 0]], SEG_SKY)
    return dict(t=t, seg=seg, second=second, T=T)


def sensor_reading(t, far=FAR, near=NEAR):
    """what a sensor with a reach writes for the distance t (its own measure: range, or depth along the axis): clamped, `far` on a miss"""
    return np.clip(t, near, far)


# ---------------------------------------------------------------- the rays
def pixel_rays():
    """fp64 unit directions [H * W, 3] of the W x H raster of a camera at identity pose (forward +x, up +z, right = forward x up = -y): the
    formula of depth_reference.camera_rays and render.camera_rays"""
    th = np.tan(np.radians(FOVY) / 2)
    u = (2 * (np.arange(W) + 0.5) / W - 1) * th * W / H
    v = (1 - 2 * (np.arange(H) + 0.5) / H) * th
    fwd, right, up = np.array([1.0, 0.0, 0.0]), np.array([0.0, -1.0, 0.0]), np.array([0.0, 0.0, 1.0])
    d = fwd[None, None] + u[None, :, None] * right[None, None] + v[:, None, None] * up[None, None]
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3)


def pixel(row, col):
    return row * W + col


CENTRE = pixel(H // 2, W // 2)
N_GENERAL = 32                                            # LiDAR rays 0 .. 31: general directions; 32 .. 37: +-x, +-y, +-z; 38 .. 41: 0.03 rad off +x
AXIS_RAYS = {"+x": 32, "-x": 33, "+y": 34, "-y": 35, "+z": 36, "-z": 37}
NEAR_X = (38, 39, 40, 41)


def lidar_pattern():
    """the [42, 3] float32 pattern given to the LiDAR: 32 directions spread evenly over the sphere (0.6 rad apart, none near a coordinate
    axis), the six coordinate axes, whose components are exact zeros and ones, and four rays 0.03 rad off +x"""
    i = np.arange(N_GENERAL)
    z = 1 - (2 * i + 1) / N_GENERAL
    rho = np.sqrt(1 - z * z)
    fib = np.stack([rho * np.cos(GOLDEN * i + 0.5), rho * np.sin(GOLDEN * i + 0.5), z], 1)
    axes = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    s, c = np.sin(0.03), np.cos(0.03)
    near_x = [[c, s, 0], [c, -s, 0], [c, 0, s], [c, 0, -s]]
    return np.concatenate([fib, axes, near_x]).astype(np.float32)


def lidar_rays(pattern=None):
    """what pgtt_lidar_create keeps of a pattern: each fp32 row normalised in double and rounded to fp32"""
    p = np.asarray(lidar_pattern() if pattern is None else pattern, np.float32).astype(np.float64)
    return f32(p / np.linalg.norm(p, axis=1, keepdims=True))


# ---------------------------------------------------------------- distances that say what a case is, from the realised numbers alone
def ray_segment_distance(o, d, a, b, reach=100.0):
    """smallest distance between the rays o + t d (0 <= t <= reach; d [P, 3]) and the segment a b: the clamped closest points of two segments"""
    d1, d2, r = d * reach, b - a, o - a
    A, E, F = np.sum(d1 * d1, -1), float(d2 @ d2), float(d2 @ r)
    Cc, Bb = d1 @ r, d1 @ d2
    den = A * E - Bb * Bb
    s = np.clip(np.where(den > 0, (Bb * F - Cc * E) / np.where(den > 0, den, 1.0), 0.0), 0.0, 1.0)
    t = (Bb * s + F) / E
    s = np.where(t < 0, np.clip(-Cc / A, 0, 1), np.where(t > 1, np.clip((Bb - Cc) / A, 0, 1), s))
    t = np.clip(t, 0.0, 1.0)
    return np.linalg.norm(o[None] + s[:, None] * d1 - (a[None] + t[:, None] * d2[None]), axis=-1)


def ray_point_distance(o, d, c, reach=100.0):
    oc = c - o
    s = np.clip(d @ oc, 0.0, reach)
    return np.linalg.norm(o[None] + s[:, None] * d - c[None], axis=-1)


def lateral(o, d, p):
    """distance of the rays d [P, 3] from a sphere's centre or a capsule's segment"""
    if p["type"] == SPHERE:
        return ray_point_distance(o, d, p["c"])
    ax = unit(p["ax"])
    return ray_segment_distance(o, d, p["c"] - p["hl"] * ax, p["c"] + p["hl"] * ax)


def origin_distance(o, p):
    """distance of the origin from a sphere's centre or a capsule's segment"""
    if p["type"] == SPHERE:
        return float(np.linalg.norm(p["c"] - o))
    ax = unit(p["ax"])
    s = np.clip((o - p["c"]) @ ax, -p["hl"], p["hl"])
    return float(np.linalg.norm(p["c"] + s * ax - o))


def box_class(o, d, p, grow):
    """(seen?, entry axis) of the rays against the box with its half extents grown by `grow` metres"""
    t, face = hit_box(o, d, p["c"], p["A"], p["h"] + grow, axis=True)
    return np.isfinite(t), np.where(np.isfinite(t), face, -1)


# ---------------------------------------------------------------- capsules
def capsule_families(default_geoms):
    """(name, r, hl) of the two shipped leg capsules (the thigh and the calf of render.default_robot_geoms) and of one fat capsule, in fp32"""
    thigh = next(g for g in default_geoms if g["type"] == CAPSULE and g["body"] == 2)
    calf = next(g for g in default_geoms if g["type"] == CAPSULE and g["body"] == 3)
    fams = [("thigh", thigh["size"][0], thigh["size"][1]), ("calf", calf["size"][0], calf["size"][1]), ("fat", 0.05, 0.2)]
    return [(n, float(f32(r)), float(f32(hl))) for n, r, hl in fams]


def place_capsule(d, ax, r, hl, k, dist, s0=0.0):
    """The capsule geom of axis `ax` whose centre lies `dist` from ORIGIN and whose axis the ray along d passes at the lateral distance k r, the
    closest approach at the axial coordinate s0 of the capsule: the offset is along d x ax, perpendicular to both, so that for every angle
    between the two the distance of the ray from the SEGMENT is k r (|s0| < hl)"""
    cr = np.cross(d, ax)
    e1 = cr / np.linalg.norm(cr) if np.linalg.norm(cr) > 1e-12 else perpendiculars(d)[0]
    c = (dist + s0 * float(d @ ax)) * d + K_REALISED[k] * r * e1 - s0 * ax
    return geom(CAPSULE, c, quat_z_to(ax), [r, hl])


def capsule_case(d, r, hl, theta, k, end, dist, n=0, axis_aligned=False):
    """One case of the sweep for the ray along d: the axis at angle theta to the ray, tilted in a direction that changes with the case number n;
    end = +1: the ray comes from the A end (c - hl ax), -1: from the B end.  -> dict(geom, prim, hit, theta, lateral: the two as realised)"""
    p, q = perpendiculars(d)
    e2 = np.cos(GOLDEN * n) * p + np.sin(GOLDEN * n) * q
    ax = end * (d if axis_aligned else np.cos(theta) * d + np.sin(theta) * e2)
    g = place_capsule(d, ax, r, hl, k, dist, s0=0.0 if axis_aligned else 0.5 * hl * ((n % 3) - 1))
    prim = realise_geom(g)
    return dict(geom=g, prim=prim, hit=k <= 0.9, k=k, end=end, dist=dist, asked=theta,
                theta=float(np.arctan2(np.linalg.norm(np.cross(d, prim["ax"])), abs(d @ prim["ax"]))), lateral=float(lateral(ORIGIN, d[None], prim)[0]))


def pack_sweep(dirs, families, general, miss_rays, axis_rays, name):
    """The capsule sweep over a sensor's rays `dirs`, packed into scenes of at most MAX_GEOM capsules, each capsule on a ray of its own: ANGLES x
    OFFSETS x both ends x DISTANCES for every family on the `general` rays, and for the first family a capsule exactly along each of
    `axis_rays` (rays along coordinate axes: every product of the quadratic is an exact zero) with the same offsets, ends and distances.
    miss_rays: the rays a miss may be put on.  A capsule goes to the first free ray of the current scene that no other capsule of the scene comes
    near (1.25 r and more from every other ray), so that each ray sees only its own.
    -> scenes: dict(name, geoms, terrain=None, check [rays], own [the geom each checked ray sees, -1: none], cases [the capsule_case dicts])"""
    todo = []
    for fam, r, hl in families:
        for dist in DISTANCES:
            for end in (1, -1):
                for theta in ANGLES:
                    for k in OFFSETS:
                        todo.append(dict(fam=fam, r=r, hl=hl, theta=theta, k=k, end=end, dist=dist, pin=None))
    fam, r, hl = families[0]
    pinned = [dict(fam=fam + " on an axis", r=r, hl=hl, theta=0.0, k=k, end=end, dist=dist) for dist in DISTANCES for end in (1, -1) for k in OFFSETS]
    for i, job in enumerate(pinned):                                                     # spread among the others: a scene has few axis rays
        job["pin"] = axis_rays[i % len(axis_rays)]
        todo.insert(min(len(todo), (i + 1) * 24 + i), job)
    scenes = []

    def new_scene():
        scenes.append(dict(name=f"{name} sweep {len(scenes)}", geoms=[], terrain=None, check=[], own=[], cases=[], _blocked=np.zeros(len(dirs), bool)))
        return scenes[-1]

    def try_place(sc, n, job):
        if len(sc["geoms"]) >= MAX_GEOM:
            return False
        rays = [job["pin"]] if job["pin"] is not None else [general[(n + i) % len(general)] for i in range(len(general))]
        for ray in rays:
            if ray in sc["check"] or sc["_blocked"][ray] or (job["k"] > 0.9 and ray not in miss_rays):
                continue
            case = capsule_case(dirs[ray], job["r"], job["hl"], job["theta"], job["k"], job["end"], job["dist"], n, axis_aligned=job["pin"] is not None)
            near = lateral(ORIGIN, dirs, case["prim"]) < 1.25 * job["r"]
            near[ray] = False
            if near[sc["check"]].any():
                continue
            case.update(fam=job["fam"], ray=ray)
            sc["_blocked"] |= near
            sc["geoms"].append(case["geom"]); sc["check"].append(ray); sc["own"].append(len(sc["geoms"]) - 1 if case["hit"] else -1); sc["cases"].append(case)
            return True
        return False

    for n, job in enumerate(todo):
        if not any(try_place(sc, n, job) for sc in scenes):
            assert try_place(new_scene(), n, job), job
    for sc in scenes:
        del sc["_blocked"]
        sc["check"], sc["own"] = np.array(sc["check"]), np.array(sc["own"])
    return scenes


# ---------------------------------------------------------------- spheres
def sphere_scene(dirs, foot_radius, hit_rays, miss_ray, behind_ray, empty_ray, name):
    """The smallest shipped foot sphere with its centre 2.9 m away, where b * b - cc cancels most, the ray passing its centre at 0, 0.5 and 0.9
    radii (hit_rays) and at 1.1 radii (miss_ray); a sphere 1 m BEHIND the origin on behind_ray's line; and a sphere that HOLDS the origin.  The
    last two are seen by no ray: empty_ray looks at nothing else."""
    r = float(f32(foot_radius))
    geoms, check, own = [], [], []
    for k, ray in zip(OFFSETS, list(hit_rays) + [miss_ray]):
        d = dirs[ray]
        geoms.append(geom(SPHERE, 2.9 * d + K_REALISED[k] * r * perpendiculars(d)[0], [1, 0, 0, 0], [r]))
        check.append(ray); own.append(len(geoms) - 1 if k <= 0.9 else -1)
    geoms.append(geom(SPHERE, -1.0 * dirs[behind_ray], [1, 0, 0, 0], [0.1]))
    geoms.append(geom(SPHERE, [0.1, -0.05, 0.02], [1, 0, 0, 0], [0.3]))
    check += [behind_ray, empty_ray]; own += [-1, -1]
    return dict(name=f"{name} spheres", geoms=geoms, terrain=None, check=np.array(check), own=np.array(own))


# ---------------------------------------------------------------- boxes
def all_rays(dirs):
    return np.arange(len(dirs))


def box_scene(name, rows, check):
    return dict(name=name, geoms=[], terrain=terrain_table(rows), check=np.asarray(check), own=None)


def camera_box_scenes():
    """Boxes aligned with the camera frame, every number exact in fp32.  The centre column of the 9 x 7 raster has u = 0: no component along the
    box's y axis; the centre row has v = 0: none along its z axis; the centre pixel has both.
      inside: the camera is inside the box's y and z slabs: those axes are no constraint for the zero components
      outside: the camera is outside the y slab: the centre column misses whatever x and z say; the centre row's left half still enters
      around: the camera is inside the box, which no pixel sees"""
    cross_px = sorted({pixel(H // 2, c) for c in range(W)} | {pixel(r, W // 2) for r in range(H)})
    return [box_scene("camera box, inside both zero slabs", [([1.0, 0.0625, 4.0625], [0.25, 0.25, 0.375])], cross_px),
            box_scene("camera box, outside the y slab", [([1.0, 0.4375, 4.0625], [0.25, 0.25, 0.375])], cross_px),
            box_scene("camera box around the origin", [([0.125, -0.0625, 4.125], [0.5, 0.5, 0.5])], np.arange(W * H))]


def lidar_box_scenes(dirs):
    """the origin inside a box (the axis rays on an aligned box are test_gpu_lidar.test_axis_rays_on_an_axis_aligned_box's)"""
    return [box_scene("lidar box around the origin", [([0.125, -0.0625, 4.125], [0.5, 0.5, 0.5])], all_rays(dirs))]


# ---------------------------------------------------------------- the culls
def corner_box_scene():
    """Depth camera: a box up and to the left of the view whose nearest corner reaches 0.03 m into the corner pixel's ray at depth 1 m; its centre
    is 0.27 m outside that ray on both image axes, well outside the image, and its bounding sphere crosses the cone around the frustum at that
    corner only.  Camera x (right) = -world y, camera y (up) = world z - 4, camera z = world x."""
    d = pixel_rays()[pixel(0, 0)]
    u0, v0 = -d[1] / d[0], d[2] / d[0]
    hx, hy, hz, reach = 0.3, 0.3, 0.1, 0.03
    cam = np.array([u0 + reach - hx, v0 - reach + hy, 1.0 + hz])
    return box_scene("depth cull, box at the image corner", [(f32([cam[2], -cam[0], 4.0 + cam[1]]), [hz, hx, hy])], np.arange(W * H))


def far_scenes(check, name):
    """Near `far`, straight ahead (+x): a box and, on the torso, a sphere, whose nearest point lies at 0.98 far (seen) and at 1.02 far (reads far).
    Depth along the camera's axis and range along the LiDAR's +x ray are the same number there.  The centres lie beyond far in all four."""
    out = []
    for f in (0.98, 1.02):
        out.append(box_scene(f"{name} box at {f} far", [([f * FAR + 0.25, 0.0, 4.0], [0.25, 0.625, 0.625])], check))
        out.append(dict(name=f"{name} sphere at {f} far", geoms=[geom(SPHERE, [f * FAR + 0.25, 0.0, 0.0], [1, 0, 0, 0], [0.25])], terrain=None,
                        check=np.asarray(check), own=None))
    return out


# ---------------------------------------------------------------- the scenes of each sensor
def camera_scenes(default_geoms, foot_radius):
    """-> (sweep scenes, other scenes that the depth camera and the renderer share, scenes for the depth camera's culls)"""
    dirs = pixel_rays()
    upper = [pixel(r, c) for r in range(H // 2 + 1) for c in range(W)]                   # d.z >= 0: a miss there is sky for the renderer
    general = [p for p in range(W * H) if p != CENTRE]
    sweep = pack_sweep(dirs, capsule_families(default_geoms), general, set(upper), [CENTRE], "camera")
    spheres = sphere_scene(dirs, foot_radius, [pixel(1, 1), pixel(5, 7), pixel(3, 6)], pixel(1, 6), pixel(2, 2), pixel(0, 0), "camera")
    return sweep, [spheres] + camera_box_scenes(), [corner_box_scene()] + far_scenes(np.arange(W * H), "depth cull,")


def lidar_scenes(default_geoms, foot_radius):
    """-> (sweep scenes, the other scenes)"""
    dirs = lidar_rays()
    general = list(range(N_GENERAL))
    sweep = pack_sweep(dirs, capsule_families(default_geoms), general, set(general) | set(AXIS_RAYS.values()), list(AXIS_RAYS.values()), "lidar")
    spheres = sphere_scene(dirs, foot_radius, [0, 5, 10], 15, 20, 25, "lidar")
    return sweep, [spheres] + lidar_box_scenes(dirs) + far_scenes([AXIS_RAYS["+x"], *NEAR_X], "lidar cull,")


# ---------------------------------------------------------------- is a scene what it claims to be?  (the CPU test's condition)
def ambiguities(scene, dirs, reach=True):
    """Every reason why a checked ray of a scene could be read two ways, from the reference and the realised numbers alone; an empty list is what
    the GPU test relies on.  reach: the sensor has a `far` (the renderer has none).
      sphere, capsule: the origin is at least MARGIN outside (or, for a sphere, inside); the ray passes within 0.9 r (hit) or beyond 1.1 r (miss)
      box: growing or shrinking the half extents by MARGIN changes neither seen / unseen nor the entry face
      no two candidates along one ray within MARGIN relative; no hit within MARGIN relative of far or of near"""
    why = []
    prims, ids = scene_prims(scene)
    chk = np.asarray(scene["check"])
    d = dirs[chk]
    e = expected(scene, dirs)
    for p, pid in zip(prims, ids):
        seen = np.isfinite(hit_prim(ORIGIN, d, p))
        if p["type"] == BOX:
            (s0, f0), (s1, f1), (s2, f2) = (box_class(ORIGIN, d, p, g) for g in (0.0, MARGIN, -MARGIN))
            bad = (s0 != s1) | (s0 != s2) | (f0 != f1) | (f0 != f2)
        else:
            lat, od, r = lateral(ORIGIN, d, p), origin_distance(ORIGIN, p), p["r"]
            if p["type"] == SPHERE and od <= r - MARGIN:
                bad = seen                                                                # the origin is inside: unseen by every ray
            elif od >= r + MARGIN:
                bad = ~(((lat <= 0.9 * r) & seen) | ((lat >= 1.1 * r) & ~seen))
            else:
                bad = np.ones(len(chk), bool)
        why += [f"{scene['name']}: ray {ray} against primitive {pid}" for ray in chk[bad]]
    t, second = e["t"][chk], e["second"][chk]
    tie = np.isfinite(t) & np.isfinite(second) & (second < t * (1 + MARGIN))
    why += [f"{scene['name']}: ray {ray} has two candidates within {MARGIN} relative" for ray in chk[tie]]
    if reach:
        m = t * d[:, 0] if reach == "depth" else t
        edge = np.isfinite(m) & ((np.abs(m - FAR) < MARGIN * FAR) | (m < NEAR * (1 + MARGIN)))
        why += [f"{scene['name']}: ray {ray} reads {v} too close to near or far" for ray, v in zip(chk[edge], m[edge])]
    return why
