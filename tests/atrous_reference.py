"""float64 numpy statement of the edge-avoiding a-trous filter of p3d_denoise (include/p3d.h): the formula the GPU result is
checked against.  Not a test module: tests/test_denoise_api.py checks it on hand-made cases, tests/test_gpu_denoise.py
compares the kernel with it."""
import numpy as np

KERNEL = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])


def luma(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def atrous(rgb, normal_depth, albedo_cov, var=None, iterations=5, sigma_color=1.0, sigma_luma=4.0, sigma_normal=128.0,
           sigma_depth=1.0, sigma_albedo=0.1):
    """rgb (h, w, 3), normal_depth / albedo_cov (h, w, 4), var (h, w) or None -> (rgb', var') in float64."""
    c = np.asarray(rgb, np.float64)
    h, w = c.shape[:2]
    v = np.zeros((h, w)) if var is None else np.asarray(var, np.float64)
    nd = np.asarray(normal_depth, np.float64)
    ac = np.asarray(albedo_cov, np.float64)
    n, t, a = nd[..., :3], nd[..., 3], ac[..., :3]
    cov = ac[..., 3] != 0
    rows, cols = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for i in range(iterations):
        s = 2 ** i
        wsum = np.zeros((h, w))
        csum = np.zeros((h, w, 3))
        vsum = np.zeros((h, w))
        yp = luma(c)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qr, qc = rows + dy * s, cols + dx * s
                valid = (qr >= 0) & (qr < h) & (qc >= 0) & (qc < w)
                qr, qc = np.clip(qr, 0, h - 1), np.clip(qc, 0, w - 1)
                cq, vq = c[qr, qc], v[qr, qc]
                hk = KERNEL[dx + 2] * KERNEL[dy + 2]
                if dx == 0 and dy == 0:
                    wt = np.ones((h, w))
                else:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        wg = np.ones((h, w))
                        if sigma_normal != 0:
                            wg = wg * np.maximum(0.0, (n * n[qr, qc]).sum(-1)) ** sigma_normal
                        if sigma_depth != 0:
                            wg = wg * np.exp(-np.abs(t - t[qr, qc]) / (sigma_depth * s * t))
                        if sigma_albedo != 0:
                            wg = wg * np.exp(-((a - a[qr, qc]) ** 2).sum(-1) / sigma_albedo ** 2)
                        covq = cov[qr, qc]
                        wg = np.where(~cov & ~covq, 1.0, np.where(cov != covq, 0.0, wg))
                        if var is not None:
                            wc = np.exp(-np.abs(yp - luma(cq)) / (sigma_luma * np.sqrt(v) + 1e-4))
                        else:
                            wc = np.exp(-((c - cq) ** 2).sum(-1) * 4.0 ** i / sigma_color ** 2)
                    wt = wg * wc
                hw = np.where(valid, hk * wt, 0.0)
                wsum += hw
                csum += hw[..., None] * cq
                vsum += hw * hw * vq
        c = csum / wsum[..., None]
        v = vsum / (wsum * wsum)
    return c, v


def u8(x, gamma=1.0):
    """gamma + u8fromfloat as the render kernels do it, for gamma = 1 (float32: min(255, (uint8)(x * 255.99f)))."""
    assert gamma == 1.0
    s = np.asarray(x, np.float32) * np.float32(255.99)
    return np.where(s >= 255, 255, np.maximum(s, 0)).astype(np.uint8)
