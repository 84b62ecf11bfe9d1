"""fp64 restatement of clhip_gather_tasks_resized_crop_flip (include/clhip.h) and of data.draw_resized_crop_flip, for the tests
of the RandomResizedCrop + flip augmentation: the per-axis weight matrix of the antialiased bilinear filter, window -> resize ->
flip of one frame, a batch of them, and the draw of the windows as a plain Python loop over the same table of uniforms."""
import math

import torch


def axis_weights(n_in, n_out):
    """float64 [n_out][n_in]: row i holds the normalised triangle weights of output element i over the source elements
    (scale = n_in / n_out, sup = max(scale, 1), centre scale (i + 0.5), taps [int(c - sup + 0.5), int(c + sup + 0.5)) clipped
    to the axis)."""
    scale = float(n_in) / float(n_out)
    sup = max(scale, 1.0)
    W = torch.zeros((n_out, n_in), dtype=torch.float64)
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo, hi = max(0, int(c - sup + 0.5)), min(n_in, int(c + sup + 0.5))
        w = [max(0.0, 1.0 - abs((j - c + 0.5) / sup)) for j in range(lo, hi)]
        total = sum(w)
        for j, v in zip(range(lo, hi), w):
            W[i, j] = v / total
    return W


def taps(n_in, n_out):
    """The largest number of taps [lo, hi) of any output element of the axis."""
    scale = float(n_in) / float(n_out)
    sup = max(scale, 1.0)
    return max(min(n_in, int(scale * (i + 0.5) + sup + 0.5)) - max(0, int(scale * (i + 0.5) - sup + 0.5)) for i in range(n_out))


def resize(window, th, tw):
    """float64 [..., th, tw] of a window [..., h, w]."""
    h, w = window.shape[-2:]
    return axis_weights(h, th) @ window.double() @ axis_weights(w, tw).t()


def resized_crop_flip(frame, top, left, h, w, flip, th, tw):
    """torchvision's crop, resize, then hflip of one frame [C][Hs][Ws], in float64."""
    out = resize(frame[:, top:top + h, left:left + w], th, tw)
    return out.flip(-1) if flip else out


def restate(frames, idx, params, th, tw):
    """float64 [B][C][th][tw]: frames[idx[b]] under params[b] = (top, left, h, w, flip)."""
    return torch.stack([resized_crop_flip(frames[g], *p, th, tw) for g, p in zip(idx.tolist(), params.tolist())])


def aten(frames, idx, params, th, tw):
    """The same batch by ATen's fp32 CPU operator (what torchvision's tensor resized_crop + hflip run)."""
    import torch.nn.functional as F
    rows = []
    for g, (top, left, h, w, flip) in zip(idx.tolist(), params.tolist()):
        win = frames[g, :, top:top + h, left:left + w].float()[None]
        out = F.interpolate(win, size=(th, tw), mode="bilinear", align_corners=False, antialias=True)[0]
        rows.append(out.flip(-1) if flip else out)
    return torch.stack(rows)


def draw(n, spec, frame_hw, generator, order=None, tries=10):
    """RandomResizedCrop.get_params + the flip, sample by sample: list of (top, left, h, w, flip, accepted).  The uniforms are
    the rows of ONE torch.rand((n, 2 * tries + 3)) in float64: columns [0, tries) the areas, [tries, 2 tries) the aspects, then
    top, left, flip."""
    u = torch.rand((n, 2 * tries + 3), generator=generator, dtype=torch.float64).tolist()
    out = []
    for k in range(n):
        if spec.extents is None:
            H, W = frame_hw
        else:
            H, W = spec.extents[k if order is None else int(order[k])].tolist()
        row = None
        for a in range(tries):
            area = H * W * (spec.scale[0] + u[k][a] * (spec.scale[1] - spec.scale[0]))
            l0, l1 = math.log(spec.ratio[0]), math.log(spec.ratio[1])
            aspect = math.exp(l0 + u[k][tries + a] * (l1 - l0))
            w, h = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
            if 0 < w <= W and 0 < h <= H:
                top = min(int(math.floor(u[k][2 * tries] * (H - h + 1))), H - h)
                left = min(int(math.floor(u[k][2 * tries + 1] * (W - w + 1))), W - w)
                row = [top, left, h, w, True]
                break
        if row is None:
            in_ratio = float(W) / float(H)
            if in_ratio < spec.ratio[0]:
                w, h = W, int(round(W / spec.ratio[0]))
            elif in_ratio > spec.ratio[1]:
                h, w = H, int(round(H * spec.ratio[1]))
            else:
                w, h = W, H
            w, h = min(max(w, 1), W), min(max(h, 1), H)
            row = [(H - h) // 2, (W - w) // 2, h, w, False]
        out.append(tuple(row[:4]) + (int(u[k][2 * tries + 2] < spec.p), row[4]))
    return out
