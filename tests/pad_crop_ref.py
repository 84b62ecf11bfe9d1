"""Restatement of torchvision's RandomCrop(size, padding, fill, padding_mode) -> hflip as index maps, in plain Python and torch
indexing on the CPU: what clhip_gather_tasks_pad_crop_flip is compared with, bitwise.  It is itself checked against
torch.nn.functional.pad (`oracle`, tests/test_pad_crop_cpu.py)."""
import torch
import torch.nn.functional as F

MODES = ("constant", "edge", "reflect", "symmetric")


def pad_map(s, n, mode):
    """Where coordinate s of the padded axis (unpadded origin) is taken from in [0, n); None: nowhere, it is the fill."""
    if 0 <= s < n:
        return s
    if mode == "constant":
        return None
    if mode == "edge":
        return min(max(s, 0), n - 1)
    if mode == "reflect":
        m = -s if s < 0 else 2 * (n - 1) - s
    else:
        m = -s - 1 if s < 0 else 2 * n - 1 - s
    assert 0 <= m < n, "one reflection must suffice: pad %d of extent %d, mode %s" % (s, n, mode)
    return m


def pad_limit(mode, extent):
    """The largest pad the mode takes on an axis of that extent (None: any)."""
    return {"reflect": extent - 1, "symmetric": extent}.get(mode)


def window(frame, top, left, flip, h, w, th, tw, mode, fill):
    """frame [C][Hs][Ws] whose valid part is [:h, :w]; the th x tw window at (top, left) of its padded image, then hflip.
    fill: C floats."""
    C = frame.shape[0]
    rows = [pad_map(top + y, h, mode) for y in range(th)]
    cols = [pad_map(left + x, w, mode) for x in range(tw)]
    out = torch.empty((C, th, tw), dtype=frame.dtype)
    for c in range(C):
        out[c] = float(fill[c])
    ys = [y for y, r in enumerate(rows) if r is not None]
    xs = [x for x, c in enumerate(cols) if c is not None]
    if ys and xs:
        src = frame[:, [rows[y] for y in ys]][:, :, [cols[x] for x in xs]]
        out[:, torch.tensor(ys)[:, None], torch.tensor(xs)[None, :]] = src
    return out.flip(-1) if flip else out


def restate(frames, idx, params, th, tw, mode, fill):
    """frames [n][C][Hs][Ws], params rows (top, left, flip, h, w) -> [B][C][th][tw]."""
    return torch.stack([window(frames[g], top, left, flip, h, w, th, tw, mode, fill)
                        for g, (top, left, flip, h, w) in zip(idx.tolist(), params.tolist())])


def _pad_symmetric(x, pl, pt, pr, pb):
    """cat(flip(x[..., :p]), x, flip(x[..., -p:])) per axis."""
    W = x.shape[-1]
    x = torch.cat([x[..., :pl].flip(-1), x, x[..., W - pr:].flip(-1)], -1)
    H = x.shape[-2]
    return torch.cat([x[..., :pt, :].flip(-2), x, x[..., H - pb:, :].flip(-2)], -2)


def oracle(frame, top, left, flip, h, w, th, tw, mode, fill, pads):
    """The same window by torch's own padding: F.pad (constant / replicate / reflect) or the symmetric concatenation of the
    valid part, then slicing, then flip(-1)."""
    pl, pt, pr, pb = pads
    v = frame[:, :h, :w]
    if mode == "constant":
        p = torch.stack([F.pad(v[c], (pl, pr, pt, pb), value=float(fill[c])) for c in range(v.shape[0])])
    elif mode == "symmetric":
        p = _pad_symmetric(v, pl, pt, pr, pb)
    else:
        p = F.pad(v[None], (pl, pr, pt, pb), mode="replicate" if mode == "edge" else "reflect")[0]
    out = p[:, top + pt:top + pt + th, left + pl:left + pl + tw]
    assert tuple(out.shape[1:]) == (th, tw)
    return out.flip(-1) if flip else out


# (Hs, Ws, th, tw, (pl, pt, pr, pb)) of the kernel tests; "limit": pads at the mode's limit for the 5 x 4 frame
GEOMETRIES = [
    (13, 11, 8, 7, (2, 2, 2, 2)),        # odd widths, plain path
    (20, 20, 16, 16, (4, 4, 4, 4)),      # vector stores, odd left, a 4-column group straddling each border
    (16, 16, 16, 16, (4, 4, 4, 4)),      # crop = frame, the CIFAR rule
    (8, 8, 12, 12, (2, 2, 2, 2)),        # crop larger than the frame
    (9, 40, 9, 1, (1, 0, 1, 0)),         # one column
    (12, 12, 8, 8, (1, 2, 3, 0)),        # asymmetric pads, zero on one side
    (72, 72, 70, 64, (3, 3, 3, 3)),      # two chunks of lines per channel, short last chunk
    (5, 4200, 2, 4100, (8, 2, 8, 2)),    # a line longer than a block's segment
    (5, 4, 8, 8, "limit"),               # pads at the mode's limit
    (5, 4, 4, 4, (6, 6, 6, 6)),          # constant / edge only: a window lying entirely in the padding
]


def pads_of(geometry, mode):
    """The pads of a geometry under a mode, or None where the mode does not take it."""
    Hs, Ws, th, tw, pads = geometry
    if pads == "limit":
        lim_h, lim_w = pad_limit(mode, Hs), pad_limit(mode, Ws)
        if lim_h is None:
            lim_h, lim_w = Hs, Ws                      # constant / edge take any pad: the symmetric limit
        pads = (lim_w, lim_h, lim_w, lim_h)
    lim_h, lim_w = pad_limit(mode, Hs), pad_limit(mode, Ws)
    if lim_h is not None and (max(pads[1], pads[3]) > lim_h or max(pads[0], pads[2]) > lim_w):
        return None
    return pads


def cases():
    """(id, geometry, mode, pads) of every geometry a mode takes."""
    out = []
    for g in GEOMETRIES:
        for mode in MODES:
            pads = pads_of(g, mode)
            if pads is not None:
                out.append(("%dx%d_to_%dx%d_%s" % (g[0], g[1], g[2], g[3], mode), g, mode, pads))
    return out


def corner_rows(h, w, th, tw, pads):
    """9 parameter rows (top, left, flip, h, w): top and left at both ends of their ranges, odd offsets, strictly inside the
    image where the image holds the window (no border touched), mixed flips."""
    pl, pt, pr, pb = pads
    t0, t1, l0, l1 = -pt, h + pb - th, -pl, w + pr - tw
    assert t0 <= t1 and l0 <= l1

    def mid(a, b, inner_hi):
        """A corner inside [0, inner_hi] when the image holds the window, else the middle of the range."""
        return min(max(inner_hi // 2, 0), inner_hi) if inner_hi >= 0 else (a + b) // 2

    it, il = mid(t0, t1, h - th), mid(l0, l1, w - tw)
    clamp_t, clamp_l = (lambda v: min(max(v, t0), t1)), (lambda v: min(max(v, l0), l1))
    rows = [[t0, l0, 0], [t1, l1, 1], [t0, l1, 1], [t1, l0, 0], [it, il, 0], [it, il, 1], [clamp_t(t0 + 1), clamp_l(l0 + 1), 1],
            [clamp_t(t1 - 1), clamp_l(l1 - 3), 0], [clamp_t(-1), clamp_l(1), 1]]
    return torch.tensor([r + [h, w] for r in rows], dtype=torch.int32)
