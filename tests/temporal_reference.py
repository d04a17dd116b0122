"""float64 numpy statement of p3d_temporal (include/p3d.h "Temporal accumulation"): the formula the GPU result is checked
against.  Not a test module: tests/test_temporal_api.py checks it on hand-made cases, tests/test_gpu_temporal.py compares the
kernels with it.

Two things are float32 by definition, and are emulated here operation by operation: the pixel-centre direction d (the render
kernels' primary_ray, csrc/device_core.hpp) and the state kept between frames (colour, n, m1, m2), which is rounded to float32
at the end of every frame.  The parameters are float32 fields.  Everything else is evaluated in float64."""
import numpy as np

F = np.float32
LUMA = (0.2126, 0.7152, 0.0722)


def _cam(c):
    """A p3d.Camera (ctypes) or a dict with the same fields -> dict of float32 arrays / scalars."""
    g = (lambda k: c[k]) if isinstance(c, dict) else (lambda k: getattr(c, k))
    out = {k: np.array(list(g(k)), F) for k in ("eye", "u", "v", "n")}
    out.update({k: F(g(k)) for k in ("w", "h", "plane_dist", "focal_ratio", "aperture")})
    out.update(res_x=int(g("res_x")), res_y=int(g("res_y")))
    return out


def same_camera(a, b):
    """Every field bit for bit (what makes the kernel map every pixel onto itself)."""
    a, b = _cam(a), _cam(b)
    for k in ("eye", "u", "v", "n"):
        if not np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)):
            return False
    for k in ("w", "h", "plane_dist", "focal_ratio", "aperture"):
        if np.asarray(a[k]).view(np.uint32) != np.asarray(b[k]).view(np.uint32):
            return False
    return a["res_x"] == b["res_x"] and a["res_y"] == b["res_y"]


def primary_dirs(cam, w, h):
    """primary_ray(cam, x + 0.5, y + 0.5) of every pixel, in float32 as the kernels compute it -> (h, w, 3) float32."""
    c = _cam(cam)
    x = np.arange(w, dtype=F) + F(0.5)
    y = np.arange(h, dtype=F) + F(0.5)
    psx = (c["w"] * (x / F(c["res_x"]) - F(0.5)))[None, :]
    psy = (c["h"] * (y / F(c["res_y"]) - F(0.5)))[:, None]
    psz = -c["plane_dist"]
    comp = [(c["u"][i] * psx + c["v"][i] * psy) + c["n"][i] * psz for i in range(3)]
    comp = [np.broadcast_to(a, (h, w)).astype(F) for a in comp]
    length = np.sqrt((comp[0] * comp[0] + comp[1] * comp[1]) + comp[2] * comp[2])
    inv = F(1.0) / length
    return np.stack([a * inv for a in comp], -1).astype(F)


def _dot(a, b):
    return (a[..., 0] * b[0] + a[..., 1] * b[1]) + a[..., 2] * b[2]


class TemporalReference:
    """One p3d_temporal object.  run() takes a frame and returns (rgb, var, history, info) in float64.  info["ambiguous"]
    marks the pixels whose colour or history hangs on a test within `margin` of its threshold, or reads a tap that did in an
    earlier frame; info["var_ambiguous"] the same for the variance (a short history reads its 7x7 neighbourhood);
    info["var_scale"] the largest m2 the pixel's variance is computed from, which its rounding scales with."""

    def __init__(self, w, h, margin=1e-9):
        self.w, self.h, self.margin = int(w), int(h), margin
        self.reset()

    def reset(self):
        self.prev = None
        self.state = None

    def run(self, cam, rgb, normal_depth, albedo_cov, alpha=0.2, alpha_moments=0.2, max_history=32.0, depth_tolerance=0.1,
            normal_tolerance=0.9, variance_min_history=4, sigma_normal=128.0, sigma_depth=1.0):
        alpha, alpha_moments, max_history, depth_tolerance, normal_tolerance, sigma_normal, sigma_depth = (
            float(F(v)) for v in (alpha, alpha_moments, max_history, depth_tolerance, normal_tolerance, sigma_normal, sigma_depth))
        w, h, mg = self.w, self.h, self.margin
        rgb = np.asarray(rgb, F).astype(np.float64)
        nd = np.asarray(normal_depth, F)
        ac = np.asarray(albedo_cov, F)
        cov = ac[..., 3] > 0
        npv = nd[..., :3].astype(np.float64)
        t = nd[..., 3].astype(np.float64)
        rows, cols = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        W = np.zeros((h, w))
        hist = np.zeros((h, w, 4))  # R, G, B, n
        hmom = np.zeros((h, w, 2))  # m1, m2
        amb = np.zeros((h, w), bool)
        if self.prev is not None:
            q = _cam(self.prev)
            pc, pm, pnd, ptaint = self.state
            d = primary_dirs(cam, w, h).astype(np.float64)
            eye, qeye = _cam(cam)["eye"].astype(np.float64), q["eye"].astype(np.float64)
            e = np.where(cov[..., None], (eye + t[..., None] * d) - qeye, d)
            dist = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
            if same_camera(cam, self.prev):
                px, py = cols.astype(np.float64), rows.astype(np.float64)
                front = np.ones((h, w), bool)
            else:
                qu, qv, qn = (q[k].astype(np.float64) for k in ("u", "v", "n"))
                a, b, cc = _dot(e, qu), _dot(e, qv), _dot(e, qn)
                front = cc < 0
                amb |= np.abs(cc) <= mg * dist
                with np.errstate(divide="ignore", invalid="ignore"):
                    s = -np.float64(q["plane_dist"]) / cc
                    px = ((a * s) / np.float64(q["w"]) + 0.5) * q["res_x"] - 0.5
                    py = ((b * s) / np.float64(q["h"]) + 0.5) * q["res_y"] - 0.5
                # (no margin on the floors: the kernel evaluates these float64 expressions in this order, so px and py are
                # the same bits there, and a tap whose weight a floor flips is ~1e-8 - a pan along an image axis does that
                # to every pixel)
            inside = front & (px > -1) & (px < w) & (py > -1) & (py < h)
            px, py = np.where(inside, px, 0.0), np.where(inside, py, 0.0)
            x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
            fx, fy = px - x0, py - y0
            np2 = (npv[..., 0] * npv[..., 0] + npv[..., 1] * npv[..., 1]) + npv[..., 2] * npv[..., 2]
            for k in range(4):
                qx, qy = x0 + (k & 1), y0 + (k >> 1)
                wk = (fx if k & 1 else 1.0 - fx) * (fy if k >> 1 else 1.0 - fy)
                valid = inside & (wk != 0) & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                qxc, qyc = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                valid &= cov == (pm[qyc, qxc, 2] > 0)
                nq = pnd[qyc, qxc].astype(np.float64)
                dtest = np.abs(nq[..., 3] - dist) - depth_tolerance * dist
                nn = (npv[..., 0] * nq[..., 0] + npv[..., 1] * nq[..., 1]) + npv[..., 2] * nq[..., 2]
                nq2 = (nq[..., 0] * nq[..., 0] + nq[..., 1] * nq[..., 1]) + nq[..., 2] * nq[..., 2]
                ntest = nn - (normal_tolerance * np.sqrt(np2)) * np.sqrt(nq2)
                amb |= valid & cov & ((np.abs(dtest) <= mg * dist) | ((dtest <= 0) & (np.abs(ntest) <= mg)))
                valid &= ~cov | ((dtest <= 0) & (ntest >= 0))
                amb |= valid & ptaint[qyc, qxc]
                W += np.where(valid, wk, 0.0)
                hist += np.where(valid[..., None], wk[..., None] * pc[qyc, qxc].astype(np.float64), 0.0)
                hmom += np.where(valid[..., None], wk[..., None] * pm[qyc, qxc, :2].astype(np.float64), 0.0)
            amb |= np.abs(W - 1e-3) <= mg
        Y = (LUMA[0] * rgb[..., 0] + LUMA[1] * rgb[..., 1]) + LUMA[2] * rgb[..., 2]
        has = W >= 1e-3
        with np.errstate(divide="ignore", invalid="ignore"):
            n = np.where(has, np.minimum(hist[..., 3] / W + 1.0, max_history), 1.0).astype(F).astype(np.float64)
            a = np.maximum(alpha, 1.0 / n)
            am = np.maximum(alpha_moments, 1.0 / n)
            out = np.where(has[..., None], (1.0 - a[..., None]) * (hist[..., :3] / W[..., None]) + a[..., None] * rgb, rgb)
            m1 = np.where(has, (1.0 - am) * (hmom[..., 0] / W) + am * Y, Y)
            m2 = np.where(has, (1.0 - am) * (hmom[..., 1] / W) + am * (Y * Y), Y * Y)
        var = np.maximum(0.0, m2 - m1 * m1)
        col_s = np.concatenate([out, n[..., None]], -1).astype(F)  # the state the next frame reads, in float32
        mom_s = np.stack([m1, m2, ac[..., 3].astype(np.float64)], -1).astype(F)
        # the spatial estimate of the short histories, over this frame's stored moments
        short = n < F(variance_min_history)
        sm = mom_s.astype(np.float64)
        ws, s1, s2 = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
        scale = np.zeros((h, w))
        near_amb = np.zeros((h, w), bool)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                qr, qc = rows + dy, cols + dx
                inb = (qr >= 0) & (qr < h) & (qc >= 0) & (qc < w)
                qr, qc = np.clip(qr, 0, h - 1), np.clip(qc, 0, w - 1)
                if dx == 0 and dy == 0:
                    wg = np.ones((h, w))
                else:
                    covq = cov[qr, qc]
                    wg = np.ones((h, w))
                    with np.errstate(divide="ignore", invalid="ignore"):
                        if sigma_normal != 0:
                            wg = wg * np.maximum(0.0, (npv * npv[qr, qc]).sum(-1)) ** sigma_normal
                        if sigma_depth != 0:
                            wg = wg * np.exp(-np.abs(t - t[qr, qc]) / (sigma_depth * t))
                    wg = np.where(~cov & ~covq, 1.0, np.where(cov != covq, 0.0, wg))
                wg = np.where(inb, wg, 0.0)
                ws += wg
                s1 += wg * sm[qr, qc, 0]
                s2 += wg * sm[qr, qc, 1]
                scale = np.maximum(scale, np.where(wg > 0, np.abs(sm[qr, qc, 1]), 0.0))
                near_amb |= inb & amb[qr, qc]
        with np.errstate(divide="ignore", invalid="ignore"):
            var = np.where(short, np.maximum(0.0, s2 / ws - (s1 / ws) ** 2), var)
        self.prev = cam
        self.state = (col_s, mom_s, nd.copy(), amb)
        return out, var, n, dict(ambiguous=amb, var_ambiguous=amb | (short & near_amb),
                                 var_scale=np.where(short, scale, np.abs(m2)), W=W)
