"""Inputs and references for the image encoder's training kernels (``csrc/image_encoder*.{hip,inc}``): plain torch on the
host, shared by ``test_conv_cases_cpu.py`` (which certifies them without a GPU) and ``test_gpu_image_encoder_scale.py``
(which runs the kernels on them where one workgroup walks several images, bands or half-images).

The references are torch in fp64 (the truth) and the same calls in fp32 (the yardstick of the error rule
``max(1e-4, 3 x yardstick)``).  The weight and bias gradients are contractions of ARBITRARY ``(g, act)`` tensors, not
derivatives of a network, so a kernel can be handed inputs whose answer is known without arithmetic: the impulse cases.
"""
import collections
import functools

import torch
import torch.nn.functional as F

IMG = 32
FLOOR = 1e-4                     # the project's bar: max(FLOOR, 3 x yardstick)
G_IMPULSE, ACT_IMPULSE = 3.0, 0.75
DW_IMPULSE = G_IMPULSE * ACT_IMPULSE   # 2.25: every operand of the f16 split and every sum of a few of them is exact
WGRAD_LAYERS = ((32, 32), (16, 32), (8, 16))   # (co, ci) of the 3x3 layers; the stem is (32, 1) with k = 5


def bar(yardstick: float) -> float:
    return max(FLOOR, 3.0 * yardstick)


def max_err(got, want) -> float:
    """Largest absolute difference over the reference's largest entry."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).abs().max()) / max(1e-30, float(want.abs().max()))


# ------------------------------------------------------------------------------ references
def wgrad_ref(g, act, k, dtype=torch.float64):
    """``dW[co][ci][ky][kx] = sum_n,y,x g[n][co][y][x] act[n][ci][y + ky - k // 2][x + kx - k // 2]``."""
    co, ci = g.shape[1], act.shape[1]
    return torch.nn.grad.conv2d_weight(act.detach().cpu().to(dtype), (co, ci, k, k), g.detach().cpu().to(dtype), padding=k // 2)


def bgrad_ref(g, dtype=torch.float64):
    return g.detach().cpu().to(dtype).sum((0, 2, 3))


def dgrad_chain_ref(weights, a1, h, a2, a3, g_a4, dtype=torch.float64):
    """The four masked transposed convolutions of ``mmf_image_convs_train_backward``: ``weights = (w2a, w2b, w3, w4)`` of
    the forward layers; returns the pre-activation gradients ``g3, g2, gh, g1`` with
    ``g1 = (g2 + dgrad(block1)(gh)) [a1 > 0]``."""
    c = lambda t: t.detach().cpu().to(dtype)
    w2a, w2b, w3, w4 = [c(w) for w in weights]
    m = lambda t: (t.detach().cpu() > 0).to(dtype)
    g3 = F.conv_transpose2d(c(g_a4), w4, padding=1) * m(a3)
    g2 = F.conv_transpose2d(g3, w3, padding=1) * m(a2)
    gh = F.conv_transpose2d(g2, w2b, padding=1) * m(h)
    g1 = (g2 + F.conv_transpose2d(gh, w2a, padding=1)) * m(a1)
    return g3, g2, gh, g1


def convs_forward_ref(params, images, dtype=torch.float64):
    """The five-layer stack: ``params = (w1, w2a, w2b, w3, w4, b1, b2a, b2b, b3, b4)``, ``images (N, 32, 32)`` ->
    ``a1, h, a2, a3, a4``."""
    w1, w2a, w2b, w3, w4, b1, b2a, b2b, b3, b4 = [p.detach().cpu().to(dtype) for p in params]
    x = images.detach().cpu().to(dtype)[:, None]
    a1 = torch.relu(F.conv2d(x, w1, b1, padding=2))
    h = torch.relu(F.conv2d(a1, w2a, b2a, padding=1))
    a2 = torch.relu(a1 + F.conv2d(h, w2b, b2b, padding=1))
    a3 = torch.relu(F.conv2d(a2, w3, b3, padding=1))
    a4 = F.conv2d(a3, w4, b4, padding=1)
    return a1, h, a2, a3, a4


def encoder_params(seq):
    """``(w1, w2a, w2b, w3, w4, b1, b2a, b2b, b3, b4)`` of a ``layers.image_encoder`` stack."""
    convs = [seq[0], seq[2].block1, seq[2].block2, seq[3], seq[5]]
    return [c.weight for c in convs] + [c.bias for c in convs]


# ------------------------------------------------------------------------------ dense inputs
@functools.lru_cache(maxsize=None)
def dense_wgrad_case(N, co, ci, k):
    """``g`` Gaussian, ``act = relu(Gaussian)`` (the stem: an image clamped to [-1, 1]); ``dw, db`` in fp64 and the fp32
    yardsticks.  Built once, handed out read-only."""
    gen = torch.Generator().manual_seed(1000 * N + 10 * co + ci)
    g = torch.randn((N, co, IMG, IMG), generator=gen)
    act = torch.randn((N, ci, IMG, IMG), generator=gen)
    act = (act * 0.5).clamp(-1, 1) if ci == 1 else torch.relu(act)
    dw, db = wgrad_ref(g, act, k), bgrad_ref(g)
    y_dw = max_err(wgrad_ref(g, act, k, torch.float32), dw)
    y_db = max_err(bgrad_ref(g, torch.float32), db)
    return g, act, dw, db, y_dw, y_db


@functools.lru_cache(maxsize=None)
def dense_dgrad_acts(N, seed=0):
    """Synthetic ``a1, h, a2, a3 = relu(Gaussian)`` and a Gaussian ``g_a4`` (float32, host)."""
    gen = torch.Generator().manual_seed(4000 + 7 * N + seed)
    a1, h, a2 = [torch.relu(torch.randn((N, 32, IMG, IMG), generator=gen)) for _ in range(3)]
    a3 = torch.relu(torch.randn((N, 16, IMG, IMG), generator=gen))
    g_a4 = torch.randn((N, 8, IMG, IMG), generator=gen)
    return a1, h, a2, a3, g_a4


SEAM_YS, SEAM_XS = (0, 7, 8, 15, 16, 23, 24, 31), (0, 31)


@functools.lru_cache(maxsize=None)
def band_seam_case():
    """One ``g_a4`` impulse per image at the rows on either side of every 8-row band seam and at both image edges, in the
    first and last column; all activations 1.0, so every mask is open.  ``(a1, h, a2, a3, g_a4)``, 16 images."""
    pos = [(y, x) for y in SEAM_YS for x in SEAM_XS]
    N = len(pos)
    g_a4 = torch.zeros((N, 8, IMG, IMG))
    for n, (y, x) in enumerate(pos):
        g_a4[n, n % 8, y, x] = 1.0
    ones = lambda c: torch.ones((N, c, IMG, IMG))
    return ones(32), ones(32), ones(32), ones(16), g_a4


# ------------------------------------------------------------------------------ impulse cases of the weight gradients
# g: one entry of 3.0 at (gn, co, gy, gx); act: one entry of 0.75 at (an, ci, ay, ax).  `adjacent`: what the case states
# about itself -- whether dW[co][ci] holds 2.25 at tap (ay - gy + k // 2, ax - gx + k // 2) or is all zero.
Impulse = collections.namedtuple("Impulse", "gn gy gx an ay ax adjacent")

_SEAM_COLS = (7, 8, 15, 16, 23, 24)          # lane halves of the f16x3 kernel (8 pixels) and of the exact one (16)
POSITIONS = tuple([(y, x) for y in (0, 31) for x in (0, 31)]                      # the four corners
                  + [(y, x) for y in (15, 16) for x in (0,) + _SEAM_COLS + (31,)]  # the seam of the two half-image units
                  + [(y, x) for y in (0, 31) for x in _SEAM_COLS])                 # the column seams at the image's edge


@functools.lru_cache(maxsize=None)
def impulse_cases(N, k=3):
    """Every position of ``POSITIONS`` with every neighbour offset of a ``k x k`` kernel that falls inside the image,
    spread over the ``N`` images; then the pairs that are adjacent in MEMORY but not in the image (``adjacent=False``)."""
    r = k // 2
    out = []
    for y, x in POSITIONS:
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if 0 <= y + dy < IMG and 0 <= x + dx < IMG:
                    n = len(out) % N
                    out.append(Impulse(n, y, x, n, y + dy, x + dx, True))
    for n in range(N):
        for y in (0, 15, 16, 30):
            out.append(Impulse(n, y, 31, n, y + 1, 0, False))       # next word of memory, next row of the image
            out.append(Impulse(n, y + 1, 0, n, y, 31, False))       # and the reverse
        out.append(Impulse(n, 31, 31, n, 0, 0, None))               # act one channel on (see impulse_batches), row 0:
        out.append(Impulse(n, 31, 5, n, 0, 5, None))                # the next word, and "row 32" of the g impulse's column
        if n + 1 < N:
            out.append(Impulse(n, 31, 31, n + 1, 0, 0, False))      # the next image's first pixel
            out.append(Impulse(n + 1, 0, 0, n, 31, 31, False))
    return tuple(out)


ImpulseBatch = collections.namedtuple("ImpulseBatch", "g act dw db owners")


def _expected(placed, co, ci, k):
    """The stated answer of a batch, by the rule alone: every (g impulse, act impulse) pair of one image within the kernel's
    reach puts 2.25 at its tap of ``dW[co of g][ci of act]``; ``db[co]`` is 3.0 per g impulse of that channel."""
    r = k // 2
    dw, db = torch.zeros((co, ci, k, k), dtype=torch.float64), torch.zeros(co, dtype=torch.float64)
    for a, a_co, _ in placed:
        db[a_co] += G_IMPULSE
        for b, _, b_ci in placed:
            ty, tx = b.ay - a.gy + r, b.ax - a.gx + r
            if a.gn == b.an and 0 <= ty < k and 0 <= tx < k:
                dw[a_co, b_ci, ty, tx] += DW_IMPULSE
    return dw, db


@functools.lru_cache(maxsize=None)
def impulse_batches(N, co, ci, k=3):
    """The cases of ``impulse_cases(N, k)`` packed into launches: every case of a batch has its own output channel and
    (3x3 layers) its own input channel, so its cell ``dW[co][ci]`` holds its own answer only; what a case's ``g`` makes of
    ANOTHER case's ``act`` lands in cells no case owns and is part of the stated answer all the same.  The channel
    assignment rotates from batch to batch so that every channel is used.  A case with ``adjacent=None`` puts its ``act``
    into channel ``ci + 1`` (the next plane of memory) and owns the cell of channel ``ci``, which stays zero.
    ``owners``: ``(case, co, ci)``."""
    cases = impulse_cases(N, k)
    size = co if ci == 1 else min(co, ci)
    out = []
    for b0 in range(0, len(cases), size):
        batch, rot = cases[b0:b0 + size], b0 // size
        g, act = torch.zeros((N, co, IMG, IMG)), torch.zeros((N, ci, IMG, IMG))
        placed, owners = [], []
        for j, c in enumerate(batch):
            o = (j + rot) % co
            i = 0 if ci == 1 else (size - 1 - j + 3 * rot) % ci
            i_act = i
            if c.adjacent is None:
                if ci == 1:
                    continue                                   # the stem has one input channel: no next plane
                i_act = (i + 1) % ci
                if i_act == 0 or any(p[2] == i_act for p in placed):
                    continue                                   # channel ci + 1 must be the next plane and unowned here
            g[c.gn, o, c.gy, c.gx] += G_IMPULSE
            act[c.an, i_act, c.ay, c.ax] += ACT_IMPULSE
            placed.append((c, o, i_act))
            owners.append((c, o, i))
        dw, db = _expected(placed, co, ci, k)
        out.append(ImpulseBatch(g, act, dw, db, tuple(owners)))
    return tuple(out)


# ------------------------------------------------------------------------------ ImageConvsFunction against fp64 autograd
def image_convs_against_fp64(N, gscale, report=None):
    """``engine.ImageConvsFunction`` in the precision that is set: outputs and all ten gradients against fp64 torch autograd
    through the same layers under the kernel's own ReLU masks, 1e-4.  ``report(name, err, yardstick)``, when given, is called
    with every figure before it is asserted."""
    from multimodalfilter_amd import _abi, engine, layers

    from _tol import rel_err

    dev = torch.device("cuda:0")
    torch.manual_seed(70 + N)
    seq = layers.image_encoder(64).to(dev)
    g = torch.Generator().manual_seed(N)
    img = (torch.randn((N, 32, 32), generator=g) * 0.5).clamp(-1, 1)
    img[N // 2] = 0.0
    gout = torch.randn((N, 8, 32, 32), generator=g) * gscale
    params = engine.PackedImageEncoder(seq)._sources()[:10]
    a4 = engine.ImageConvsFunction.apply(seq, img.to(dev), *params)
    got = torch.autograd.grad(a4, params, gout.to(dev))

    # Among ~1e6 pre-activations a few sit within fp32 rounding of zero, where an fp32 forward and an
    # fp64 one take different ReLU branches (one such pixel moves a weight gradient by 1e-3): the
    # reference applies the masks of the kernel's own forward, so that only arithmetic is compared
    mk = lambda c: torch.empty((N, c, 32, 32), dtype=torch.float32, device=dev)
    k1, kh, k2, k3, k4 = mk(32), mk(32), mk(32), mk(16), mk(8)
    _abi.image_convs_train_forward(seq._mmf_packed.blob(), img.to(dev).contiguous(), k1, kh, k2, k3, k4, engine.range_flag(dev),
                                   engine.training_image_precision_code())   # the arithmetic ImageConvsFunction ran in
    m1, mh, m2, m3 = [(t > 0).double().cpu() for t in (k1, kh, k2, k3)]

    def reference(dtype):
        p = [q.detach().cpu().to(dtype).requires_grad_(True) for q in params]
        w1, w2a, w2b, w3, w4, b1, b2a, b2b, b3, b4 = p
        x = img.to(dtype)[:, None]
        a1 = F.conv2d(x, w1, b1, padding=2) * m1.to(dtype)
        h = F.conv2d(a1, w2a, b2a, padding=1) * mh.to(dtype)
        a2 = (a1 + F.conv2d(h, w2b, b2b, padding=1)) * m2.to(dtype)
        a3 = F.conv2d(a2, w3, b3, padding=1) * m3.to(dtype)
        out = F.conv2d(a3, w4, b4, padding=1)
        return out.detach(), torch.autograd.grad(out, p, gout.to(dtype))

    ref, want = reference(torch.float64)
    names = "w1 w2a w2b w3 w4 b1 b2a b2b b3 b4".split()
    yard = {}
    if report is not None:   # the figures go out beside the same autograd in fp32 on the host
        ref32, want32 = reference(torch.float32)
        yard = {n: max_err(a, b) for n, a, b in zip(names, want32, want)}
        yard["a4"] = rel_err(ref32, ref, dims=3)
    err = rel_err(a4.detach(), ref, dims=3)
    if report is not None:
        report("a4", err, yard["a4"])
    assert err < 1e-4   # every image's (8, 32, 32) feature map
    for name, a, b in zip(names, got, want):
        scale = max(1e-30, float(b.abs().max()))
        err = float((a.cpu().double() - b).abs().max()) / scale
        if report is not None:
            report(name, err, yard[name])
        assert err < 1e-4, (name, gscale)
