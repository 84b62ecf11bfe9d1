"""Shared helpers of the kernel-level parity tests (test_gpu_loss_kernels.py, test_gpu_hat_kernels.py,
test_gpu_gemm_kernels.py, test_gpu_pool_kernels.py, test_gpu_bn_kernels.py, test_gpu_packnet_kernels.py,
test_gpu_elementwise_kernels.py, test_gpu_gem_kernels.py, test_gpu_fc_chain_kernels.py, test_gpu_conv2d_kernels.py,
test_gpu_conv5x5_bs_kernels.py, test_gpu_wino_kernels.py, test_gpu_conv3x3_kernels.py, test_gpu_bs3x3_kernels.py,
test_gpu_window_chunks.py, test_window_plan_cpu.py) — test infrastructure.

The fp32-chain rule is the one of assert_fp32_parity in test_gpu_parity.py with the bounds these two files use: the device
result's distance from an fp64 evaluation of the same formula on the same float32 inputs, relative to the tensor's largest
entry, must not exceed max(base, 4 x the distance of torch's own float32 CPU evaluation).  The factor 4: device expf / logf /
powf / coshf are allowed a few ulp more than the host's, and the row sums run in another order.  Every figure is printed
before it is asserted (`MEASURED|<test id>|<what>|<device>|<float32 CPU>`), so one run with -s yields the headroom tables
kept in the docstrings of the two test files."""
import torch

LOSS_BASE = 1e-5      # what test_softmax_ce asserts
HAT_BASE = 1e-6       # what test_elementwise_regularizers_match_oracle asserts for its SGD steps
CPU_FACTOR = 4.0


def fp32_chain_check(case, what, got, ref32, ref64, base, scale=None):
    """scale: what the distances are measured against; default the fp64 reference's largest entry.  A caller passes the
    size of the terms when the result is a difference of much larger ones (BatchNorm's dz)."""
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    ref32 = torch.as_tensor(ref32).detach().double().reshape(-1)
    ref64 = torch.as_tensor(ref64).detach().double().reshape(-1)
    assert got.shape == ref64.shape == ref32.shape, (what, got.shape, ref32.shape, ref64.shape)
    assert bool(torch.isfinite(ref64).all()), what + ": the fp64 reference is not finite"
    scale = max(float(ref64.abs().max()) if scale is None else float(scale), 1e-30)
    d = (got - ref64).abs()
    e_dev = float(d.max()) / scale if bool(torch.isfinite(got).all()) else float("inf")
    e_cpu = float((ref32 - ref64).abs().max()) / scale
    print("MEASURED|%s|%s|%.3e|%.3e" % (case, what, e_dev, e_cpu))
    assert e_dev <= max(base, CPU_FACTOR * e_cpu), \
        "%s: %.3e of its scale from the fp64 value (float32 CPU: %.3e, base %.0e)" % (what, e_dev, e_cpu, base)
    return e_dev, e_cpu


def ulp_distance(a, b):
    """Largest distance in float32 units in the last place between two float32 tensors (0 <=> bitwise equal up to the sign
    of zero); NaN anywhere => a huge number."""
    a, b = a.detach().cpu().contiguous().reshape(-1), b.detach().cpu().contiguous().reshape(-1)
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape
    if a.numel() == 0:
        return 0
    if bool(torch.isnan(a).any()) or bool(torch.isnan(b).any()):
        return 1 << 40

    def key(x):                                       # monotone map of the float32 line onto the integers
        i = x.view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    return int((key(a) - key(b)).abs().max())


def bitwise_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def bit_pattern(n, bits):
    """n float32 that all hold the 32-bit pattern `bits` (a NaN with a chosen payload survives every copy bit for bit)."""
    assert 0 <= bits < 1 << 31
    return torch.full((n,), bits, dtype=torch.int32).view(torch.float32)


def all_bits(t, bits):
    return bool((t.detach().cpu().contiguous().view(torch.int32) == bits).all())


class ConvRef:
    """fp64 and float32-CPU results of one convolution layer on float32 operands x [N][C][H][W], w [K][C][R][S], dy [N][K][OH][OW]
    (zero padding `pad`, stride `stride`): y (no bias), dx, dw, db, and for each product the same product of the operands'
    absolute values (s_y, s_dx, s_dw: what a float32 rounding analysis of a dot product is measured in)."""

    def __init__(self, x, w, dy, stride, pad):
        import torch.nn.functional as F
        from torch.nn.grad import conv2d_input, conv2d_weight
        xd, wd, dyd = x.double(), w.double(), dy.double()
        self.y64 = F.conv2d(xd, wd, None, stride, pad)
        assert self.y64.shape == dy.shape, (self.y64.shape, dy.shape)
        self.s_y = F.conv2d(xd.abs(), wd.abs(), None, stride, pad)
        self.y32 = F.conv2d(x, w, None, stride, pad)
        self.dx64 = conv2d_input(x.shape, wd, dyd, stride, pad)
        self.s_dx = conv2d_input(x.shape, wd.abs(), dyd.abs(), stride, pad)
        self.dx32 = conv2d_input(x.shape, w, dy, stride, pad)
        self.dw64 = conv2d_weight(xd, w.shape, dyd, stride, pad)
        self.s_dw = conv2d_weight(xd.abs(), w.shape, dyd.abs(), stride, pad)
        self.dw32 = conv2d_weight(x, w.shape, dy, stride, pad)
        self.db64 = dyd.sum((0, 2, 3))
        self.s_db = dyd.abs().sum((0, 2, 3))


# Winograd F(2x2, 3x3) (Lavin & Gray): Y = A^T [ (G g G^T) .* (B^T d B) ] A.  The transforms add and cancel, so the direct product of
# absolute values (ConvRef.s_y) is no bound for the terms a Winograd kernel rounds; the two functions below evaluate the same
# formulas with every matrix and operand replaced by its absolute value, in fp64: what a rounding analysis of csrc/wino.hip is measured in.
WINO_BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
WINO_G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
WINO_AT = [[1, 1, 1, 0], [0, 1, -1, -1]]


def _wino_windows(t, win):
    """[N][C][H][W] -> [N][C][TH][TW][win][win]: the 4x4 input windows (win = 4, one zero ring around the map) or the 2x2 output
    tiles (win = 2) of the ceil(H/2) x ceil(W/2) tiles; what lies outside the map (tiles half outside an odd map) is zero."""
    N, C, H, W = t.shape
    TH, TW = (H + 1) // 2, (W + 1) // 2
    lead = 1 if win == 4 else 0
    p = torch.zeros((N, C, 2 * TH + 2 * lead, 2 * TW + 2 * lead), dtype=torch.float64)
    p[:, :, lead:lead + H, lead:lead + W] = t.double()
    return p.unfold(2, win, 2).unfold(3, win, 2)


def wino_magnitude(inp, g):
    """S_w[n][k][h][w] = |A^T| [ sum_c (|G| |g| |G^T|) .* (|B^T| |d| |B|) ] |A| for inp [N][Cin][H][W], g [Cout][Cin][3][3] as the
    KERNEL sees them (backward-data: inp = dy, g[c][k] = the 180-degree-rotated w[k][c]).  S_w >= conv(|inp|, |g|) element by element."""
    N, Cin, H, W = inp.shape
    Bt, G, At = (torch.tensor(m, dtype=torch.float64).abs() for m in (WINO_BT, WINO_G, WINO_AT))
    d = _wino_windows(inp.abs(), 4)                                            # [N][Cin][TH][TW][4][4]
    TH, TW = d.shape[2], d.shape[3]
    V = torch.einsum("ai,nctuij,bj->abcntu", Bt, d, Bt).reshape(16, Cin, N * TH * TW)
    Uw = torch.einsum("ar,kcrs,bs->abkc", G, g.double().abs(), G).reshape(16, g.shape[0], Cin)
    M = torch.bmm(Uw, V).reshape(4, 4, g.shape[0], N, TH, TW)
    Y = torch.einsum("ia,abkntu,jb->nktiuj", At, M, At).reshape(N, g.shape[0], 2 * TH, 2 * TW)
    return Y[:, :, :H, :W].contiguous()


def wino_wgrad_magnitude(x, dy):
    """S_wg[k][c][r][s] = |G^T| [ sum over images and tiles (|A| |dY| |A^T|) .* (|B^T| |d| |B|) ] |G| for x [N][C][H][W], dy [N][K][H][W]."""
    N, C, H, W = x.shape
    K = dy.shape[1]
    Bt, G, At = (torch.tensor(m, dtype=torch.float64).abs() for m in (WINO_BT, WINO_G, WINO_AT))
    V = torch.einsum("ai,nctuij,bj->abcntu", Bt, _wino_windows(x.abs(), 4), Bt).reshape(16, C, -1)
    D = torch.einsum("ia,nktuij,jb->abkntu", At, _wino_windows(dy.abs(), 2), At).reshape(16, K, -1)
    M = torch.bmm(D, V.transpose(1, 2)).reshape(4, 4, K, C)
    return torch.einsum("ar,abkc,bs->kcrs", G, M, G).contiguous()


class Arena:
    """Tensors packed into one flat float32 buffer, each at a 16-byte boundary or exactly one float past one, with sentinel
    gaps between them: one upload, one download, and a write outside any tensor shows in the gaps."""
    GAP = 7.25

    def __init__(self):
        self.items = []            # (offset, host tensor)
        self.size = 4

    def add(self, t, misaligned=False, fill=None):
        """t: a tensor, or with `fill` a number of floats that all start as that 32-bit pattern (bit_pattern).
        misaligned: True or 1 = one float past a 16-byte boundary; 2 = two floats past one (8-byte aligned, not 16)."""
        if fill is not None:
            t = bit_pattern(int(t), fill)
        t = t.detach().contiguous().reshape(-1).float()
        off = (self.size + 3) // 4 * 4 + 4 + int(misaligned)
        self.items.append((off, t))
        self.size = off + t.numel()
        return len(self.items) - 1

    def host(self):
        flat = torch.full((self.size + 8,), self.GAP, dtype=torch.float32)
        for off, t in self.items:
            flat[off:off + t.numel()] = t
        return flat

    def upload(self, device):
        self.dev = self.host().to(device)
        assert self.dev.data_ptr() % 16 == 0
        return self

    def ptr(self, k):
        off, t = self.items[k]
        return self.dev.data_ptr() + 4 * off

    def download(self):
        self.back = self.dev.cpu()
        return self

    def get(self, k):
        off, t = self.items[k]
        return self.back[off:off + t.numel()]

    def gaps_untouched(self):
        keep = torch.ones(self.back.numel(), dtype=torch.bool)
        for off, t in self.items:
            keep[off:off + t.numel()] = False
        return bool((self.back[keep] == self.GAP).all())


class ByteArena:
    """Arena's counterpart for uint8 tensors (PackNet's task masks, the pools' arg-max codes): one flat byte buffer, every
    tensor at an odd byte offset (or, odd=False, on a 16-byte boundary), sentinel bytes in the gaps between them."""
    GAP = 0xA5

    def __init__(self):
        self.items = []            # (offset, host tensor)
        self.size = 16

    def add(self, t, odd=True, fill=None, shift=None):
        """t: a uint8 tensor, or with `fill` a number of bytes that all start as that value.  shift: bytes past a 16-byte
        boundary (0..15), instead of what `odd` says."""
        if fill is not None:
            t = torch.full((int(t),), int(fill), dtype=torch.uint8)
        t = t.detach().contiguous().reshape(-1)
        assert t.dtype == torch.uint8
        off = (self.size + 15) // 16 * 16 + 16 + ((5 if odd else 0) if shift is None else int(shift))
        self.items.append((off, t))
        self.size = off + t.numel()
        return len(self.items) - 1

    def host(self):
        flat = torch.full((self.size + 32,), self.GAP, dtype=torch.uint8)
        for off, t in self.items:
            flat[off:off + t.numel()] = t
        return flat

    def upload(self, device):
        self.dev = self.host().to(device)
        assert self.dev.data_ptr() % 16 == 0
        return self

    def ptr(self, k):
        off, t = self.items[k]
        return self.dev.data_ptr() + off

    def download(self):
        self.back = self.dev.cpu()
        return self

    def get(self, k):
        off, t = self.items[k]
        return self.back[off:off + t.numel()]

    def gaps_untouched(self):
        keep = torch.ones(self.back.numel(), dtype=torch.bool)
        for off, t in self.items:
            keep[off:off + t.numel()] = False
        return bool((self.back[keep] == self.GAP).all())
