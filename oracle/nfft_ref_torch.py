"""The float64 restatement of ``nfft_ref.py`` in torch, device-agnostic -- TEST INFRASTRUCTURE ONLY.

Same algorithm, conventions and citations as ``oracle/nfft_ref.py`` (Gaussian window b = 4m/(3 pi), oversampling 2,
2m+2 taps per axis, shift = floor(pos*M) - m, unnormalised e^{+} / e^{-} FFTs, roll-off exp(k^2 pi m / (3 N^2)) per
axis); see that file for the reference lines restated.  Tensors in, tensors out, on the inputs' device, so that on
a GPU a 10^7-point problem on a 512^3 grid takes seconds where the numpy version takes hours.  The product never imports
this module.

``dtype=torch.float64`` (default) is the oracle.  ``dtype=torch.float32`` runs the SAME code in float32 / complex64
(fp32 atomics in the spreading, a single-precision FFT, an fp32 roll-off: the arithmetic of the reference).  That mode
is a yardstick for what single precision costs on a given problem, not an oracle; it is meant for power-of-two N, where
pos * M is exact in float32.

Memory: one point set at a time, and of its columns as many planes together as keep three copies of their grids under
``GROUP_BYTES`` (one plane for grids of 512^3 and more; small grids share one sweep over the points).  The adjoint cuts
the band out after each FFT axis and the forward pads one axis at a time, so that a call holds about two complex grids
of (2N)^d per plane of the group plus the FFT's work area (``peak_bytes``).  Spreading and gathering loop over the taps
of the leading axes with the last axis vectorised, over blocks of ``BLOCK_POINTS`` points (argument ``block``), so
temporaries are O(block * (2m+2)).
"""
import itertools
import math

import torch

BLOCK_POINTS = 1 << 20
GROUP_BYTES = 8 << 30


def _types(dtype):
    if dtype == torch.float64:
        return torch.float64, torch.complex128
    if dtype == torch.float32:
        return torch.float32, torch.complex64
    raise TypeError("dtype must be torch.float64 or torch.float32")


def _batch_info(batch, n, device):
    if batch is None:
        return None, 1  # core_cuda.cu:62-65
    batch = torch.as_tensor(batch, device=device).to(torch.int64)
    return batch, (int(batch[-1]) + 1 if n else 1)  # core_cuda.cu:60


def _point_sets(pos, bvec, B):
    """(b, index tensor or None) for every non-empty point set."""
    if bvec is None:
        if pos.shape[0]:
            yield 0, None
        return
    for b in range(B):
        sel = torch.nonzero(bvec == b).squeeze(1)
        if sel.numel():
            yield b, sel


def window_taps(pos, N, m, dtype=torch.float64, deriv=False):
    """shift [n,d] int64, psi [n,d,2m+2] (spatial_window_operations.cu:38-97) and, with ``deriv``, d psi / d pos."""
    rdt, _ = _types(dtype)
    M, W = 2 * N, 2 * m + 2
    u = pos.to(torch.float32).to(rdt) * M  # exact in fp32 for a power-of-two M
    fl = torch.floor(u)
    shift = fl.to(torch.int64) - m
    l = torch.arange(W, dtype=rdt, device=pos.device)
    t = (u - (fl - m))[:, :, None] - l
    psi = torch.exp(-(t * t) * (0.75 * math.pi / m)) * math.sqrt(0.75 / m)
    if not deriv:
        return shift, psi
    return shift, psi, -2.0 * t * (0.75 * math.pi / m) * psi * M


def phi_hat_inv(N, m, dtype=torch.float64, device=None):
    """exp(k^2 * pi*m/(3 N^2)), k = 0..N/2 (spectral_window_operations.cu:2-3, 14-43)."""
    rdt, _ = _types(dtype)
    k = torch.arange(N // 2 + 1, dtype=rdt, device=device)
    return torch.exp(k * k * (math.pi / 3.0) * m / (N * N))


def _rolloff_axis(N, m, dtype, device):
    """phi_hat_inv[|i - N/2|] for the centred index i = 0..N-1 of one axis."""
    idx = (torch.arange(N, device=device) - N // 2).abs()
    return phi_hat_inv(N, m, dtype, device)[idx]


def _band_index(N, device=None):
    """kappa = (i - N/2) mod 2N for i = 0..N-1 (spectral_window_operations.cu:78-96)."""
    return torch.remainder(torch.arange(N, device=device) - N // 2, 2 * N)


def _tap_cells(shift, M, W):
    """For every tap tuple ``ls`` of the leading d-1 axes: (ls, flat cell index [n, W] of the last axis' W taps)."""
    n, d = shift.shape
    last = torch.remainder(shift[:, d - 1:d] + torch.arange(W, device=shift.device), M)
    for ls in itertools.product(range(W), repeat=d - 1):
        base = torch.zeros(n, dtype=torch.int64, device=shift.device)
        for a, l in enumerate(ls):
            base = base * M + torch.remainder(shift[:, a] + l, M)
        yield ls, base[:, None] * M + last


def _group(C, d, N, dtype):
    """How many planes are processed together: as many as keep three copies of their grids under GROUP_BYTES."""
    csize = 16 if dtype == torch.float64 else 8
    return max(1, min(C, GROUP_BYTES // (3 * (2 * N) ** d * csize)))


def _spread_planes(g, xcols, pos, N, m, dtype, block):
    """Adds the window-weighted coefficients xcols [n, G] of G columns into the complex grids g [G, (2N)^d] (one point
    set)."""
    rdt, _ = _types(dtype)
    M, W = 2 * N, 2 * m + 2
    n, d = pos.shape
    G = g.shape[0]
    out = torch.view_as_real(g).view(G, -1)  # (re, im) interleaved: cell c of a plane is out[:, 2c], out[:, 2c+1]
    block = max(1, block // G)
    for s in range(0, n, block):
        shift, psi = window_taps(pos[s:s + block], N, m, dtype)
        xb = xcols[s:s + block].t()  # [G, nb]
        re = (xb.real if xb.is_complex() else xb).to(rdt)[:, :, None]
        im = xb.imag.to(rdt)[:, :, None] if xb.is_complex() else None
        for ls, cell in _tap_cells(shift, M, W):
            w = psi[:, d - 1, :]
            if ls:
                wo = psi[:, 0, ls[0]]
                for a in range(1, d - 1):
                    wo = wo * psi[:, a, ls[a]]
                w = wo[:, None] * w
            idx = (2 * cell).view(-1)
            out.index_add_(1, idx, (w * re).reshape(G, -1))
            if im is not None:
                out.index_add_(1, idx + 1, (w * im).reshape(G, -1))


def _gather_planes(g, pos, N, m, dtype, block, deriv=False):
    """y [n, G] = sum over taps of psi * g (spatial_window_operations.cu:214-332) for the G planes g [G, (2N)^d]; with
    ``deriv`` also dy [n, d, G], the same sums with the window's derivative along each axis in turn."""
    rdt, cdt = _types(dtype)
    M, W = 2 * N, 2 * m + 2
    n, d = pos.shape
    G = g.shape[0]
    gflat = g.reshape(G, -1)
    y = torch.zeros((n, G), dtype=cdt, device=pos.device)
    dy = torch.zeros((n, d, G), dtype=cdt, device=pos.device) if deriv else None
    block = max(1, block // G)
    for s in range(0, n, block):
        taps = window_taps(pos[s:s + block], N, m, dtype, deriv)
        shift, psi = taps[0], taps[1]
        dpsi = taps[2] if deriv else None
        for ls, cell in _tap_cells(shift, M, W):
            vals = gflat[:, cell]  # [G, nb, W]
            s0 = (vals * psi[:, d - 1, :]).sum(dim=2)
            wo = torch.ones((), dtype=rdt, device=pos.device)
            for a, l in enumerate(ls):
                wo = wo * psi[:, a, l]
            y[s:s + block] += (wo * s0).t()
            if deriv:
                dy[s:s + block, d - 1] += (wo * (vals * dpsi[:, d - 1, :]).sum(dim=2)).t()
                for a in range(d - 1):
                    wa = torch.ones((), dtype=rdt, device=pos.device)
                    for b, l in enumerate(ls):
                        wa = wa * (dpsi[:, b, l] if b == a else psi[:, b, l])
                    dy[s:s + block, a] += (wa * s0).t()
    return (y, dy) if deriv else y


def _grid_to_band(g, N, m, dtype):
    """Unnormalised e^{+} FFT of the grids g [G, (2N)^d], the band [G, N^d] cut out and the roll-off applied, one axis at
    a time."""
    d = g.dim() - 1
    kap = _band_index(N, g.device)
    f1 = _rolloff_axis(N, m, dtype, g.device)
    for a in reversed(range(d)):
        g = torch.fft.ifft(g, dim=1 + a, norm="forward")  # core_cuda.cu:254-272
        shape = [1] * (d + 1)
        shape[1 + a] = N
        g = g.index_select(1 + a, kap) * f1.reshape(shape)
    return g


def _band_to_grid(v, m, dtype):
    """Roll-off, zero padding to (2N)^d and the unnormalised e^{-} FFT of the bands v [G, N^d], one axis at a time."""
    d = v.dim() - 1
    N = v.shape[1]
    kap = _band_index(N, v.device)
    f1 = _rolloff_axis(N, m, dtype, v.device)
    for a in range(d):
        shape = [1] * (d + 1)
        shape[1 + a] = N
        v = v * f1.reshape(shape)
    for a in range(d):
        shape = list(v.shape)
        shape[1 + a] = 2 * N
        z = torch.zeros(shape, dtype=v.dtype, device=v.device)
        z.index_copy_(1 + a, kap, v)
        del v
        v = torch.fft.fft(z, dim=1 + a)  # core_cuda.cu:432-450
        del z
    return v


def _ncols(cols):
    C = 1
    for s in cols:
        C *= int(s)
    return C


def spread(x, pos, batch, N, m, dtype=torch.float64, block=None):
    """Adjoint gridding: g [B, C, M..M] complex (spatial_window_operations.cu:103-211)."""
    _, cdt = _types(dtype)
    block = block or BLOCK_POINTS
    n, d = pos.shape
    C = _ncols(x.shape[1:])
    x2 = x.reshape(n, C)
    bvec, B = _batch_info(batch, n, pos.device)
    g = torch.zeros((B, C) + (2 * N,) * d, dtype=cdt, device=pos.device)
    G = _group(C, d, N, dtype)
    for b, sel in _point_sets(pos, bvec, B):
        pb, xb = (pos, x2) if sel is None else (pos[sel], x2[sel])
        for c in range(0, C, G):
            _spread_planes(g[b, c:c + G], xb[:, c:c + G], pb, N, m, dtype, block)
    return g


def nfft_adjoint(x, pos, batch=None, N=16, m=3, real_output=False, dtype=torch.float64, block=None):
    """Restates nfft_adjoint_cuda (core_cuda.cu:144-336).  Returns [B, N..N, *cols]."""
    _, cdt = _types(dtype)
    block = block or BLOCK_POINTS
    n, d = pos.shape
    cols = tuple(x.shape[1:])
    C = _ncols(cols)
    x2 = x.reshape(n, C)
    bvec, B = _batch_info(batch, n, pos.device)
    y = torch.zeros((B,) + (N,) * d + (C,), dtype=cdt, device=pos.device)
    G = _group(C, d, N, dtype)
    for b, sel in _point_sets(pos, bvec, B):
        pb, xb = (pos, x2) if sel is None else (pos[sel], x2[sel])
        for c in range(0, C, G):
            g = torch.zeros((min(G, C - c),) + (2 * N,) * d, dtype=cdt, device=pos.device)
            _spread_planes(g, xb[:, c:c + G], pb, N, m, dtype, block)
            y[b, ..., c:c + G] = _grid_to_band(g, N, m, dtype).movedim(0, -1)
            del g
    y = y.reshape((B,) + (N,) * d + cols)
    return y.real.clone() if real_output else y


def _forward_planes(x, pos, batch, m, dtype):
    """Yields (sel, points of the set, first column c, grids [G, (2N)^d]) for every non-empty point set and every
    group of columns."""
    _, cdt = _types(dtype)
    n, d = pos.shape
    B, N = x.shape[0], x.shape[1]
    C = _ncols(x.shape[1 + d:])
    xr = x.reshape((B,) + (N,) * d + (C,))
    bvec, B2 = _batch_info(batch, n, pos.device)
    assert B2 == B, "Input mismatch"
    G = _group(C, d, N, dtype)
    for b, sel in _point_sets(pos, bvec, B):
        pb = pos if sel is None else pos[sel]
        for c in range(0, C, G):
            yield sel, pb, c, _band_to_grid(xr[b, ..., c:c + G].movedim(-1, 0).to(cdt), m, dtype)


def nfft_forward(x, pos, batch=None, m=3, real_output=False, dtype=torch.float64, block=None):
    """Restates nfft_forward_cuda (core_cuda.cu:340-531).  x [B, N..N, *cols] -> [n, *cols]."""
    _, cdt = _types(dtype)
    block = block or BLOCK_POINTS
    n, d = pos.shape
    N = x.shape[1]
    cols = tuple(x.shape[1 + d:])
    y = torch.zeros((n, _ncols(cols)), dtype=cdt, device=pos.device)
    for sel, pb, c, g in _forward_planes(x, pos, batch, m, dtype):
        yb = _gather_planes(g, pb, N, m, dtype, block)
        if sel is None:
            y[:, c:c + g.shape[0]] = yb
        else:
            y[sel, c:c + g.shape[0]] = yb
        del g
    y = y.reshape((n,) + cols)
    return y.real.clone() if real_output else y


def forward_pos_grad(xhat, pos, batch, m, real_output, w, dtype=torch.float64, block=None):
    """dpos [n, d] = sum_cr w[i, cr] d Fr[i, cr] / d pos[i, a], Fr the real columns of nfft_forward (C with
    real_output, else 2C: re, im interleaved): the gather with the window's derivative,
    d/dpos_a prod_b psi(t_b) = M psi'(t_a) prod_{b != a} psi(t_b),  psi'(t) = -2 t (0.75 pi / m) psi(t)."""
    rdt, _ = _types(dtype)
    block = block or BLOCK_POINTS
    n, d = pos.shape
    N = xhat.shape[1]
    C = _ncols(xhat.shape[1 + d:])
    w2 = w.reshape(n, C, 1 if real_output else 2).to(rdt)
    dpos = torch.zeros((n, d), dtype=rdt, device=pos.device)
    for sel, pb, c, g in _forward_planes(xhat, pos, batch, m, dtype):
        _, dy = _gather_planes(g, pb, N, m, dtype, block, deriv=True)  # [ns, d, G]
        wb = (w2 if sel is None else w2[sel])[:, None, c:c + g.shape[0], :]
        del g
        contrib = dy.real * wb[..., 0]
        if not real_output:
            contrib = contrib + dy.imag * wb[..., 1]
        contrib = contrib.sum(dim=2)
        if sel is None:
            dpos += contrib
        else:
            dpos[sel] += contrib
    return dpos


def nfft_fastsum(x, coeffs, sources, targets=None, source_batch=None, target_batch=None, batch=None, m=3,
                 dtype=torch.float64, block=None):
    """Restates nfft_fastsum_cuda (core_cuda.cu:535-852): adjoint at the sources, g_hat *= coeffs on the band
    (spectral_window_operations.cu:269-402), forward at the targets; real part when x is real."""
    rdt, cdt = _types(dtype)
    if targets is None:
        targets, target_batch = sources, source_batch
    if batch is not None:
        source_batch = target_batch = batch
    N, d = coeffs.shape[0], coeffs.dim()
    y = nfft_adjoint(x, sources, source_batch, N=N, m=m, dtype=dtype, block=block)
    y = y * coeffs.to(cdt if coeffs.is_complex() else rdt).reshape((1,) + tuple(coeffs.shape) + (1,) * (y.dim() - 1 - d))
    out = nfft_forward(y, targets, target_batch, m=m, dtype=dtype, block=block)
    return out if x.is_complex() else out.real.clone()


def peak_bytes(d, N, m, n, planes=1, dtype=torch.float64, block=None):
    """Upper estimate of the device memory one call of nfft_adjoint / nfft_forward / forward_pos_grad holds at its
    peak: three complex grids of (2N)^d (the FFT's input, its output and its work area) for every plane of a group, the
    band of all ``planes`` = B*C (point set, column) pairs, the per-point result and the tap temporaries of one block
    of points."""
    rsize = 8 if dtype == torch.float64 else 4
    csize = 2 * rsize
    block = min(block or BLOCK_POINTS, max(n, 1))
    W = 2 * m + 2
    grids = 3 * _group(planes, d, N, dtype) * (2 * N) ** d * csize
    band = planes * N ** d * csize
    per_point = n * (planes * csize + d * (4 + rsize + csize))
    taps = block * (3 * d * W * rsize + W * (2 * 8 + 4 * csize))
    return grids + band + per_point + taps
