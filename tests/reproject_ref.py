"""The reprojection post-process restated in NumPy: DESIGN.md 4.10, written from the reference's shaders (all-is-cubes-gpu/src/shaders/rt-copy.wgsl:73-223
rt_reproject_vertex / rt_reproject_fragment under a LessEqual depth test, shaders/resampling.wgsl:119-176 gap_fill_downsample / gap_fill_upsample through
mip_ping.rs:261-400 with 12 levels and one repetition) and not from the kernel. Every operand is np.float32 and every operation rounds once, in the order
the shaders write them; aic_reproject_split must give these bits.

Colour is handled as uint16 (f16 bit patterns) [H, W, 4], depth as float32 [H, W] whose sign bit marks a UI pixel."""
import numpy as np

F = np.float32
RATIO_CAP = F(8.0)  # decision 3 (AIC_REPROJECT_RATIO_CAP)
MAX_LEVELS = 12     # raytrace_to_texture.rs:331
MARKER = np.array([0, 0, 0, 0xBC00], np.uint16)  # (0, 0, 0, -1): "nothing known"
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
# Output pixels examined around a sprite's centre when the frame is too large to examine all of them. A covered pixel has qx^2 + qy^2 <= 0.33, so
# |fx - ox| <= sqrt(0.33) kx = sqrt(0.33) * 4 * ratio / W in NDC, which is sqrt(0.33) * 2 * ratio <= 9.2 pixels at the cap; 13 leaves room for the
# centre's own rounding.
REACH = 13


def geometry(width, height):
    """(L, (T0x, T0y), scratch bytes): mip_ping.rs:460-481 on the frame's own size; the scratch is keys and R (8 bytes a pixel each), mips 1 .. L-1
    (8 bytes a texel) and four 8-byte counters."""
    if width == 0 or height == 0:
        return 0, (0, 0), 0
    levels = min(MAX_LEVELS, (min(width, height).bit_length() - 1) + 1)
    d = 1 << levels
    t0 = (-(-width // d) * d, -(-height // d) * d)
    texels = sum((t0[0] >> k) * (t0[1] >> k) for k in range(1, levels))
    return levels, t0, width * height * 16 + texels * 8 + 32


def _f16(bits):
    return bits.view(np.float16).astype(F)


def valid(texels):
    """gf_valid on [..., 4] uint16 texels"""
    return _f16(np.ascontiguousarray(texels[..., 3])) > F(-0.5)


def _lin(t, zw):
    a, b, c, g = (F(v) for v in zw)
    return -(t * a + b) / (t * c + g)


def splat(color, depth, matrix, ipzw):
    """Stage A. matrix: 16 float32, column-major ([c*4+r]). Returns dict(R [H,W,4] u16, D [H,W] f32, n_splats, n_dropped, n_gaps)."""
    H, W = depth.shape
    m = np.asarray(matrix, F).reshape(4, 4).T  # m[r][c]
    depth = np.ascontiguousarray(depth, F)
    with np.errstate(all="ignore"):
        rw, rh = F(1) / F(W), F(1) / F(H)
        sy, sx = np.mgrid[0:H, 0:W]
        tcx = (sx.astype(F) + F(0.5)) * rw
        tcy = (sy.astype(F) + F(0.5)) * rh
        nx = tcx * F(2) - F(1)
        ny = -(tcy * F(2) - F(1))
        e = depth
        ui = (e.view(np.uint32) >> np.uint32(31)) != 0  # decision 1: the sign bit, so that -0.0 is a UI pixel
        nan = np.isnan(e)
        d = np.abs(e)
        h = [((m[r, 0] * nx + m[r, 1] * ny) + m[r, 2] * d) + m[r, 3] for r in range(4)]
        in_front = h[3] > F(0)  # decision 2: w = 0 is dropped too
        ox, oy, oz = h[0] / h[3], h[1] / h[3], h[2] / h[3]
        ratio = _lin(d, ipzw) / _lin(oz, ipzw)
        world_ok = ~ui & ~nan & in_front & np.isfinite(ratio) & (ratio > F(0))
        ratio = np.minimum(ratio, RATIO_CAP)
        is_ui = ui & ~nan
        ox = np.where(is_ui, nx, ox)
        oy = np.where(is_ui, ny, oy)
        oz = np.where(is_ui, F(0), oz)
        ratio = np.where(is_ui, F(1), ratio).astype(F)
        draw = world_ok | is_ui
        ozc = np.minimum(np.maximum(oz, F(0)), F(1))
        kx = (F(4) * rw) * ratio
        ky = (F(4) * rh) * ratio

        s = np.flatnonzero(draw.reshape(-1))
        ox, oy, ozc, kx, ky = (a.reshape(-1)[s].astype(F) for a in (ox, oy, ozc, kx, ky))
        keys = np.full(W * H, NO_KEY, np.uint64)
        low = (np.uint64(0xFFFFFFFF) - s.astype(np.uint64))

        def test(px, py, sel):
            """output pixels (px, py) (int arrays, inside the frame) against the sprites sel"""
            fx = (px.astype(F) + F(0.5)) * rw * F(2) - F(1)
            fy = -((py.astype(F) + F(0.5)) * rh * F(2) - F(1))
            qx = (fx - ox[sel]) / kx[sel]
            qy = (fy - oy[sel]) / ky[sel]
            d2 = qx * qx + qy * qy
            cover = (qy >= F(-0.5)) & (qy <= F(1.0) - F(1.7320508) * np.abs(qx)) & (d2 <= F(0.33))
            z = np.minimum(ozc[sel] + d2 * F(0.0125), F(1.0))
            key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low[sel]
            np.minimum.at(keys, (py * W + px)[cover], key[cover])

        everyone = np.arange(len(s))
        if W <= 2 * REACH + 1 and H <= 2 * REACH + 1:  # every output pixel against every sprite
            for py in range(H):
                for px in range(W):
                    test(np.full(len(s), px), np.full(len(s), py), everyone)
        else:
            # a centre that is not finite covers nothing (q is infinite or NaN); the others are examined REACH pixels around the pixel the centre is in
            fin = np.isfinite(ox) & np.isfinite(oy)
            bx = np.clip(np.floor((ox.astype(np.float64) + 1.0) * 0.5 * W), -1e9, 1e9).astype(np.int64)
            by = np.clip(np.floor((1.0 - oy.astype(np.float64)) * 0.5 * H), -1e9, 1e9).astype(np.int64)
            for dy in range(-REACH, REACH + 1):
                for dx in range(-REACH, REACH + 1):
                    px, py = bx + dx, by + dy
                    sel = np.flatnonzero(fin & (px >= 0) & (px < W) & (py >= 0) & (py < H))
                    if len(sel):
                        test(px[sel], py[sel], sel)

    gap = keys == NO_KEY
    winner = (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
    winner[gap] = 0
    R = np.where(gap[:, None], MARKER[None, :], color.reshape(-1, 4)[winner]).astype(np.uint16)
    zbits = (keys >> np.uint64(32)).astype(np.uint32)
    dbits = zbits | (depth.reshape(-1).view(np.uint32)[winner] & np.uint32(0x80000000))
    D = np.where(gap, F(1.0).view(np.uint32), dbits).astype(np.uint32).view(F)
    return {"R": R.reshape(H, W, 4), "D": D.reshape(H, W), "n_splats": int(draw.sum()), "n_dropped": int(W * H - draw.sum()), "n_gaps": int(gap.sum())}


def _mirror(i, n):
    m = np.mod(i, 2 * n)
    return np.where(m >= n, 2 * n - 1 - m, m)


def fill(c, src, xs, ys, wc):
    """fill(c, list): c [..., 4] u16; the list is src at (xs[k], ys[k]) -- MirrorRepeat -- with weight wc for k = 0 and 1 for the rest."""
    h, w = src.shape[:2]
    acc = np.zeros(c.shape, F)
    for k in range(5):
        t = src[_mirror(ys[k], h), _mirror(xs[k], w)]
        v = valid(t)
        wt = F(wc) if k == 0 else F(1)
        rgb = _f16(np.ascontiguousarray(t[..., :3]))
        acc[..., :3] = np.where(v[..., None], acc[..., :3] + rgb * wt, acc[..., :3])
        acc[..., 3] = np.where(v, acc[..., 3] + wt, acc[..., 3])
    with np.errstate(all="ignore"):
        avg = (acc / acc[..., 3:4]).astype(np.float16).view(np.uint16)  # nearest even, overflow to infinity
    out = np.where((acc[..., 3] > F(0.5))[..., None], avg, MARKER)
    return np.where(valid(c)[..., None], c, out).astype(np.uint16)


def _cross(x, y, step=1):
    return [x, x + step, x - step, x, x], [y, y, y, y + step, y - step]


def gap_fill(R):
    """Stage B. Returns (levels, t0, stages): stages is the list of (name, k, mip k as that stage leaves it)."""
    H, W = R.shape[:2]
    L, (t0x, t0y), _ = geometry(W, H)
    stages = []
    mips = [None] * L
    j, i = np.mgrid[0:t0y, 0:t0x]
    bx, by = ((2 * i + 1) * W) // (2 * t0x), ((2 * j + 1) * H) // (2 * t0y)
    mips[0] = fill(R[by, bx], R, *_cross(bx, by), 1.0)
    stages.append(("down", 0, mips[0].copy()))
    for k in range(1, L):
        j, i = np.mgrid[0:t0y >> k, 0:t0x >> k]
        bx, by = 2 * i + 1, 2 * j + 1
        mips[k] = fill(mips[k - 1][by, bx], mips[k - 1], *_cross(bx, by), 1.0)
        stages.append(("down", k, mips[k].copy()))
    for k in range(L - 2, 0, -1):
        j, i = np.mgrid[0:t0y >> k, 0:t0x >> k]
        c = mips[k - 1][2 * j + 1, 2 * i + 1]  # decision 4: a point on a texel boundary takes the texel it is the lower corner of
        # floor((2i+1)/4 + {0, +1/2, -1/2}) = floor((2i + {1, 3, -1}) / 4), floors towards minus infinity
        xs = [(2 * i + 1) // 4, (2 * i + 3) // 4, (2 * i - 1) // 4, (2 * i + 1) // 4, (2 * i + 1) // 4]
        ys = [(2 * j + 1) // 4, (2 * j + 1) // 4, (2 * j + 1) // 4, (2 * j + 3) // 4, (2 * j - 1) // 4]
        mips[k] = fill(c, mips[k + 1], xs, ys, 2.0)
        stages.append(("up", k, mips[k].copy()))
    if L >= 2:  # upsample 0: both inputs are mip 1 (mip_ping.rs:353)
        j, i = np.mgrid[0:t0y, 0:t0x]
        hx, hy = i >> 1, j >> 1
        mips[0] = fill(mips[1][hy, hx], mips[1], *_cross(hx, hy, 2), 2.0)
        stages.append(("up", 0, mips[0].copy()))
    return L, (t0x, t0y), stages


def reproject(color, depth, matrix, ipzw, flags=0):
    """The whole post-process. Returns dict(R, D, levels, t0, stages, color, depth, n_splats, n_dropped, n_gaps, n_unfilled)."""
    out = splat(color, depth, matrix, ipzw)
    out.update(finish(out["R"], flags))
    out["depth"] = out["D"]
    return out


def finish(R, flags=0, filled=None):
    """Gap fill and final store of a splat image; `filled` = a gap_fill(R) result to reuse."""
    H, W = R.shape[:2]
    L, (t0x, t0y), stages = filled if filled is not None else gap_fill(R)
    mip0 = stages[-1][2] if L >= 2 else stages[0][2]
    y, x = np.mgrid[0:H, 0:W]
    final = mip0[((2 * y + 1) * t0y) // (2 * H), ((2 * x + 1) * t0x) // (2 * W)]  # decision 5: the final store samples mip 0 at the pixel's centre
    if flags & 1:  # AIC_REPROJECT_KEEP_SPLATS
        final = np.where(valid(R)[..., None], R, final)
    final = np.ascontiguousarray(final, np.uint16)
    return {"levels": L, "t0": (t0x, t0y), "stages": stages, "color": final, "n_unfilled": int((~valid(final)).sum())}


# ---- cameras for the tests: a wgpu-style perspective projection (depth 0 at the near plane, 1 at the far plane), column-vector convention, f64
def perspective(fov_y_deg, aspect, near, far):
    f = 1.0 / np.tan(np.radians(fov_y_deg) / 2.0)
    p = np.zeros((4, 4))
    p[0, 0], p[1, 1] = f / aspect, f
    p[2, 2], p[2, 3] = far / (near - far), near * far / (near - far)
    p[3, 2] = -1.0
    return p


def view(yaw=0.0, position=(0.0, 0.0, 0.0)):
    """world -> eye for a camera at `position` turned by `yaw` radians about y"""
    c, s = np.cos(yaw), np.sin(yaw)
    rot = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1.0]])  # eye -> world
    tr = np.eye(4)
    tr[:3, 3] = position
    return np.linalg.inv(tr @ rot)


def reprojection(proj, view_old, view_new):
    """(matrix [16] f32 column-major, ipzw [4] f32): clip_new = P V_new (P V_old)^-1 clip_old"""
    m = proj @ view_new @ np.linalg.inv(proj @ view_old)
    ip = np.linalg.inv(proj)
    return m.T.reshape(16).astype(F), np.array([ip[2, 2], ip[2, 3], ip[3, 2], ip[3, 3]], F)
