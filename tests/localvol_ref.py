"""numpy restatement, in 80-bit arithmetic, of the local volume constraint (include/topopt_amd.h: tp_localvol), and the checks
of the device against it that tests/test_gpu_localvol.py, its child processes and the slab worker share.  Not a test module.

    N_e = { j : |c_j - c_e| < R }  (strict, truncated at the boundary),  conn = max_d ceil(R / h_d) - 1, at most half the mesh
    cnt_e = |N_e|,  rb_e = (sum_{j in N_e} rho_j) / cnt_e
    S = sum_e rb_e^p,  pn = (S / n)^(1/p),  g = pn / alpha - 1
    dg/drho_j = sum_{e in N_j} c_e,  c_e = t_e^(p-1) / (alpha n cnt_e),  t_e = rb_e / pn;  pn = 0: c = 0

It is a brute-force loop over the (2 conn + 1)^3 offsets and does nothing but these formulas."""
import math

import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53


def stencil_width(ne, h, R):
    c = max(int(math.ceil(R / hd)) - 1 for hd in h)
    return max(min(c, ne[0] // 2, ne[1] // 2, ne[2] // 2), 0)


def offsets(ne, h, R):
    """(di, dj, dk) of the ball, distances formed as the weight table of the library forms them (double, sqrt, strict <)"""
    c = stencil_width(ne, h, R)
    out = []
    for dk in range(-c, c + 1):
        for dj in range(-c, c + 1):
            for di in range(-c, c + 1):
                if math.sqrt((di * h[0]) * (di * h[0]) + (dj * h[1]) * (dj * h[1]) + (dk * h[2]) * (dk * h[2])) < R:
                    out.append((di, dj, dk))
    return out


def ball_sum(f, ne, offs):
    """out_e = sum over the offsets of f at e + offset, where that lies inside the mesh; f flat, x fastest"""
    ex, ey, ez = ne
    a = np.asarray(f).reshape(ez, ey, ex)
    out = np.zeros_like(a)
    for di, dj, dk in offs:
        x0, x1 = max(0, -di), min(ex, ex - di)
        y0, y1 = max(0, -dj), min(ey, ey - dj)
        z0, z1 = max(0, -dk), min(ez, ez - dk)
        if x0 < x1 and y0 < y1 and z0 < z1:
            out[z0:z1, y0:y1, x0:x1] += a[z0 + dk:z1 + dk, y0 + dj:y1 + dj, x0 + di:x1 + di]
    return out.ravel()


def reference(rho, ne, h, R, alpha, p, dtype=LD):
    """-> dict(cnt, rb, rb_max, S, pn, g, dgdx)"""
    offs = offsets(ne, h, R)
    n = ne[0] * ne[1] * ne[2]
    rho = np.asarray(rho).astype(dtype)
    cnt = ball_sum(np.ones(n, dtype=dtype), ne, offs)
    rb = ball_sum(rho, ne, offs) / cnt
    S = (rb ** dtype(p)).sum()
    pn = (S / n) ** (1 / dtype(p)) if S != 0 else dtype(0)
    g = pn / dtype(alpha) - 1
    if pn != 0:
        c = (rb / pn) ** dtype(p - 1) / (dtype(alpha) * n * cnt)
    else:
        c = np.zeros(n, dtype=dtype)
    return dict(cnt=cnt, rb=rb, rb_max=rb.max(), S=S, pn=pn, g=g, dgdx=ball_sum(c, ne, offs))


# ---- the fields of the tests (element order: x fastest) ----
def field(kind, ne, seed=3):
    ex, ey, ez = ne
    n = ex * ey * ez
    k, j, i = np.meshgrid(np.arange(ez), np.arange(ey), np.arange(ex), indexing="ij")
    if kind == "random":
        return np.random.default_rng(seed).uniform(0.0, 1.0, n)
    if kind == "checker":   # 0/1 checkerboard of 4^3 blocks
        return (((i // 4) + (j // 4) + (k // 4)) % 2).astype(np.float64).ravel()
    if kind == "half":      # exactly 0 on half the mesh
        f = np.random.default_rng(seed + 1).uniform(0.0, 1.0, n).reshape(ez, ey, ex)
        f[:, :, : ex // 2] = 0.0
        return f.ravel()
    raise ValueError(kind)


def bounds(conn, p):
    """the bounds of the issue for a stencil width and an exponent: rb absolute; pn, g relative; dgdx relative to its maximum"""
    taps = (2 * conn + 1) ** 3
    b_rb = (taps + 8) * U53
    return dict(taps=taps, rb=b_rb, pn=p * b_rb + 64 * U53, dgdx=(p + 1) * b_rb * 2)


def check_against_reference(tp, ne, h, R, kind, p, alpha=0.6, expect_kernel=None, tag=""):
    """One mesh, one field, one exponent on cuda:0 against reference(): checks 1-5 of tests/test_gpu_localvol.py, then rhobar and
    dgdx row by row, each relative to its own value (tests/design_rowwise.py; its fields are accepted here as well).  Every
    figure is printed with its bound before anything is asserted.  Returns the device results."""
    import torch
    from tests import design_rowwise as dr
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cuda()
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, tuple(h))
    try:
        lv = tp.LocalVolume(grid, R)
        conn = stencil_width(ne, h, R)
        case = dr.lv_case(tuple(ne), tuple(h), R, kind, p, alpha)
        rho, ref = case["rho"], case["ref"]
        b = bounds(conn, p)
        x = dev(rho)
        rb, dg, rb2 = grid.elem_vec(), grid.elem_vec(), grid.elem_vec()
        g, pn, mx = lv.Constraint(x, alpha, p, dgdx=dg, rhobar=rb)
        kern = lv.last_kernel()
        lv.Mean(x, rb2)
        g2, pn2, mx2 = lv.Constraint(x, alpha, p)          # forward only
        cnt = lv.count().cpu().numpy()
        rb_h, rb2_h, dg_h = rb.cpu().numpy(), rb2.cpu().numpy(), dg.cpu().numpy()
        e_rb = float(np.abs(rb_h.astype(LD) - ref["rb"]).max())
        e_pn = float(abs(LD(pn) - ref["pn"]) / ref["pn"]) if ref["pn"] != 0 else abs(pn)
        e_g = float(abs(LD(g) - ref["g"]) / abs(ref["g"]))
        e_mx = float(abs(LD(mx) - ref["rb_max"]))
        dmax = float(np.abs(ref["dgdx"]).max())
        e_dg = float(np.abs(dg_h.astype(LD) - ref["dgdx"]).max() / dmax) if dmax != 0 else float(np.abs(dg_h).max())
        euler = (rho.astype(LD) * dg_h.astype(LD)).sum()
        e_eu = float(abs(euler - LD(pn) / LD(alpha)))
        b_eu = b["dgdx"] * pn / alpha
        print("%s%s %s p=%g conn %d (%d taps) kernel %d: cnt %s; rb %.3e (bound %.3e); pn %.3e, g %.3e (bound %.3e); rb_max %.3e "
              "(bound %.3e); dgdx %.3e (bound %.3e); Euler %.3e (bound %.3e)"
              % (tag, "x".join(map(str, ne)), kind, p, conn, b["taps"], kern,
                 "equal" if np.array_equal(cnt, ref["cnt"].astype(np.float64)) else "DIFFERS", e_rb, b["rb"], e_pn, e_g, b["pn"],
                 e_mx, b["rb"], e_dg, b["dgdx"], e_eu, b_eu), flush=True)
        assert lv.stencil_width == conn
        if expect_kernel is not None:
            assert kern in expect_kernel, "the ball sum ran kernel %d, the case is about %r" % (kern, expect_kernel)
        assert np.array_equal(cnt, ref["cnt"].astype(np.float64))                    # 1
        assert e_rb <= b["rb"]                                                       # 2
        if kind == "checker":   # exact integer sums, one division: the bits of the division in double
            s_int = np.rint((ref["rb"] * ref["cnt"]).astype(np.float64))
            assert np.array_equal(rb_h, s_int / cnt)
        assert np.array_equal(rb_h, rb2_h)                  # Mean and Constraint: the same ball sum
        assert e_pn <= b["pn"] and e_g <= b["pn"] and e_mx <= b["rb"]                # 3
        assert (g2, pn2, mx2) == (g, pn, mx)                # the forward-only call: the same values
        assert e_dg <= b["dgdx"]                                                     # 4
        assert e_eu <= b_eu                                                          # 5
        got = dr.lv_hold(case, rb_h, dg_h, tag=tag)
        print("    row-wise, each row relative to itself, achieved c (bound): rhobar %.2f (%g), dgdx %.2f (%g)"
              % (got["rb"], case["c"][0], got["dgdx"], case["c"][1]), flush=True)
        return dict(g=g, pn=pn, mx=mx, rb=rb_h, dgdx=dg_h, cnt=cnt, kernel=kern, rowwise=got)
    finally:
        grid.close()
