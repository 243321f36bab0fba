"""The image encoder's kernels where ONE workgroup walks several images, bands or half-images and carries state from one
to the next (loop-carried accumulators, LDS planes chosen by parity, register prefetch) -- the regime ``bench.py`` always
runs them in and the rest of the suite almost never.  Inputs and fp64 references: ``_conv_cases.py`` (certified on the host by
``test_conv_cases_cpu.py``).  Sizes derive from the device's CU count ``C``; every buffer a kernel writes is handed over full
of NaN.

Exact conditions: impulse answers, power-of-two scaling, two calls giving the same bits, rows against the same rows of a
smaller call.  Dense comparisons: largest absolute difference over the reference's largest entry, at most
``max(1e-4, 3 x yardstick)``, the yardstick being the same contraction in fp32 torch on the host against fp64; every figure
is printed (``IMGSCALE group case output kernel / yardstick``) before it is asserted: ``-s | grep IMGSCALE``."""
import functools

import pytest
import torch

import _conv_cases as cc

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X (-m gpu on the GPU box)")
    return torch.device("cuda:0")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=_dev())


def _held(group, case, output, err, yard):
    print(f"IMGSCALE {group} {case} {output} {err:.2e} / {yard:.2e}", flush=True)
    assert err <= cc.bar(yard), (group, case, output, err, yard)


# ============================================================================== A. weight-gradient kernels
LAYERS = [("exact", co, ci) for co, ci in cc.WGRAD_LAYERS] + [("exact", 32, 1)] + [("f16x3", co, ci) for co, ci in cc.WGRAD_LAYERS]
LAYER_IDS = [f"{kind}_{co}x{ci}" for kind, co, ci in LAYERS]


def _n_blocks(N):
    return sorted({1, 2, 5, 2 * N, 2 * N + 3})


def _wgrad(kind, g, act, n_blocks, absmax=None):
    """One call of the kernel under test with NaN-filled outputs: ``dw, db, partial, partial_b``."""
    from multimodalfilter_amd import _abi, engine

    co, ci = g.shape[1], act.shape[1]
    k = 5 if ci == 1 else 3
    partial, partial_b, dw, db = _nan(n_blocks, 9, 32, 32), _nan(n_blocks, 32), _nan(co, ci, k, k), _nan(co)
    if kind == "f16x3":
        gm = g.abs().max().reshape(1) if absmax is None else torch.tensor([absmax], dtype=torch.float32, device=g.device)
        _abi.conv_weight_grads_h(g, act, gm, partial, partial_b, engine.range_flag(g.device), n_blocks, dw, db)
    else:
        _abi.conv_weight_grads(g, act, partial, partial_b, n_blocks, dw, db)
    return dw, db, partial, partial_b


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("kind,co,ci", LAYERS, ids=LAYER_IDS)
def test_wgrad_dense_matches_fp64_for_every_split(kind, co, ci, N):
    """``dw`` and ``db`` against fp64 whether one workgroup walks all ``2 N`` half-images (``n_blocks = 1``), several walk a
    few each, each has one, or some have none -- whose slots must come out as zeros; two calls give the same bits."""
    dev = _dev()
    k = 5 if ci == 1 else 3
    g, act, dw64, db64, y_dw, y_db = cc.dense_wgrad_case(N, co, ci, k)
    gd, ad = g.to(dev), act.to(dev)
    live = 1024 if ci == 1 else 9216   # the stem's slot is [co 32][tap 32] at the head of the workgroup's slot
    for nb in _n_blocks(N):
        dw, db, partial, partial_b = _wgrad(kind, gd, ad, nb)
        case = f"{kind} {co}x{ci} N={N} n_blocks={nb}"
        _held("A", case, "dw", cc.max_err(dw, dw64), y_dw)
        _held("A", case, "db", cc.max_err(db, db64), y_db)
        slots = partial.reshape(nb, -1)[:, :live]
        assert not torch.isnan(slots).any() and not torch.isnan(partial_b).any()
        if nb > 2 * N:   # idle workgroups
            assert not slots[2 * N:].any() and not partial_b[2 * N:].any()
        dw2, db2, partial2, partial_b2 = _wgrad(kind, gd, ad, nb)
        assert torch.equal(dw, dw2) and torch.equal(db, db2)
        assert torch.equal(slots, partial2.reshape(nb, -1)[:, :live]) and torch.equal(partial_b, partial_b2)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("kind,co,ci", LAYERS, ids=LAYER_IDS)
def test_wgrad_impulses_are_exact_for_every_split(kind, co, ci, N):
    """One ``g`` entry of 3.0 against one activation of 0.75 per case: 2.25 at the case's tap, zero everywhere else, ``db`` 3.0
    -- exactly, in both kernels (every operand of the f16 split is exact at ``g_absmax = 3``), at the corners, across the
    lane-half seams in x, across the seam of the two half-image units in y, and for pairs that are neighbours in memory only."""
    dev = _dev()
    k = 5 if ci == 1 else 3
    for b in cc.impulse_batches(N, co, ci, k):
        gd, ad = b.g.to(dev), b.act.to(dev)
        want_dw, want_db = b.dw.float().to(dev), b.db.float().to(dev)
        for nb in _n_blocks(N):
            dw, db, _, _ = _wgrad(kind, gd, ad, nb, absmax=cc.G_IMPULSE)
            if not torch.equal(dw, want_dw):
                bad = (dw != want_dw).nonzero()[0].tolist()
                owner = [c for c, o, i in b.owners if o == bad[0] and (ci == 1 or i == bad[1])]
                pytest.fail(f"{kind} {co}x{ci} N={N} n_blocks={nb}: dw{bad} = {float(dw[tuple(bad)])}, "
                            f"stated {float(want_dw[tuple(bad)])}; case {owner}")
            assert torch.equal(db, want_db), (nb, db.tolist())


@pytest.mark.parametrize("co,ci", cc.WGRAD_LAYERS)
def test_wgrad_f16x3_scale_is_an_exact_power_of_two(co, ci):
    """``dw(2^k g)`` with ``g_absmax`` scaled to match equals ``2^k dw(g)`` bit for bit at k = +-20 (and ``db`` with it): the
    operand scale is a power of two taken from ``g_absmax``'s exponent.  All-zero ``g`` with ``g_absmax = 0``: zeros."""
    dev = _dev()
    N, nb = 3, 5
    g, act = [t.to(dev) for t in cc.dense_wgrad_case(N, co, ci, 3)[:2]]
    dw, db, _, _ = _wgrad("f16x3", g, act, nb)
    for k in (20, -20):
        s = 2.0 ** k
        dws, dbs, _, _ = _wgrad("f16x3", g * s, act, nb)
        assert torch.equal(dws, dw * s) and torch.equal(dbs, db * s), k
    dwz, dbz, _, _ = _wgrad("f16x3", torch.zeros_like(g), act, nb, absmax=0.0)
    assert not dwz.any() and not dbz.any() and not torch.isnan(dwz).any() and not torch.isnan(dbz).any()


def test_wgrad_f16x3_raises_the_range_flag_and_the_exact_kernel_does_not():
    """One activation of 7e4 (beyond the f16 range) makes the operand split inexact: the f16x3 kernel says so through the
    device status word; the exact kernel takes no flag and leaves it alone."""
    from multimodalfilter_amd import _abi, engine

    dev = _dev()
    g, act = [t.to(dev) for t in cc.dense_wgrad_case(3, 32, 32, 3)[:2]]
    act = act.clone()
    act[2, 17, 16, 8] = 7e4
    engine.check_range(dev)
    try:
        _wgrad("exact", g, act, 5)
        engine.check_range(dev)       # nothing raised it
        _wgrad("f16x3", g, act, 5)
        with pytest.raises(_abi.MmfError, match="f16x3 operand range"):
            engine.check_range(dev)
        engine.check_range(dev)       # and the check cleared it
    finally:
        engine.range_flag(dev).zero_()


@pytest.mark.parametrize("kind", ["exact", "f16x3"])
def test_wgrad_refuses_unsupported_shapes(kind):
    from multimodalfilter_amd import _abi

    dev = _dev()
    g, act = torch.zeros((1, 32, 32, 32), device=dev), torch.zeros((1, 16, 32, 32), device=dev)
    with pytest.raises(_abi.MmfError):
        _wgrad(kind, g, act, 2)                                   # (co, ci) = (32, 16) is no layer of the stack
    with pytest.raises(_abi.MmfError):
        _wgrad(kind, g, torch.zeros_like(g), 0)                   # n_blocks = 0


# ============================================================================== B. data-gradient chains
@functools.lru_cache(maxsize=None)
def _encoder(seed=11):
    from multimodalfilter_amd import layers

    torch.manual_seed(seed)
    return layers.image_encoder(64).to(_dev())


def _dgrad_weights():
    return [p.detach().cpu() for p in cc.encoder_params(_encoder())[1:5]]


@functools.lru_cache(maxsize=None)
def _dgrad_reference(N):
    """fp64 ``g3, g2, gh, g1`` of the dense case and the fp32 yardsticks, once per size for both kernels."""
    acts = cc.dense_dgrad_acts(N)
    want = cc.dgrad_chain_ref(_dgrad_weights(), *acts)
    yard = [cc.max_err(a, b) for a, b in zip(cc.dgrad_chain_ref(_dgrad_weights(), *acts, dtype=torch.float32), want)]
    return want, yard


def _dgrad(kind, acts_dev, g_a4):
    """``g3, g2, gh, g1, scratch`` of one call with NaN-filled outputs."""
    from multimodalfilter_amd import _abi, engine

    a1, h, a2, a3 = acts_dev
    N = g_a4.shape[0]
    blob = engine.packed_image_encoder(_encoder()).backward_blob()
    g1, gh, g2, g3 = _nan(N, 32, 32, 32), _nan(N, 32, 32, 32), _nan(N, 32, 32, 32), _nan(N, 16, 32, 32)
    scratch = None
    if kind == "f16x3":
        scratch = _nan(4)
        _abi.image_convs_train_backward_h(blob, a1, h, a2, a3, g_a4, g1, gh, g2, g3, scratch)
    else:
        _abi.image_convs_train_backward(blob, a1, h, a2, a3, g_a4, g1, gh, g2, g3)
    return g3, g2, gh, g1, scratch


def _dgrad_sizes():
    return [1, 2, _cus() // 2 + 75]   # the last: 8 N bands on 2 C workgroups, about 300 of them take a second band


@pytest.mark.parametrize("size", [0, 1, 2], ids=["N=1", "N=2", "N=C/2+75"])
@pytest.mark.parametrize("kind", ["exact", "f16x3"])
def test_dgrad_chain_matches_fp64(kind, size):
    """``g3, g2, gh, g1`` against the four masked transposed convolutions in fp64.  f16x3: the four scale words equal the
    largest magnitudes of the tensors they describe bit for bit, and the chain on ``2^k g_a4`` is ``2^k`` x the chain on
    ``g_a4`` bit for bit at k = +-20."""
    dev = _dev()
    N = _dgrad_sizes()[size]
    acts = [t.to(dev) for t in cc.dense_dgrad_acts(N)]
    want, yard = _dgrad_reference(N)
    *acts_dev, g_a4 = acts
    got = _dgrad(kind, acts_dev, g_a4)
    for name, a, b, y in zip(("g3", "g2", "gh", "g1"), got, want, yard):
        _held("B", f"{kind} N={N}", name, cc.max_err(a, b), y)
    again = _dgrad(kind, acts_dev, g_a4)
    assert all(torch.equal(a, b) for a, b in zip(got[:4], again[:4]))
    if kind == "f16x3":
        g3, g2, gh, g1, scratch = got
        tops = torch.stack([g3.abs().max(), g2.abs().max(), gh.abs().max(), g_a4.abs().max()])
        assert torch.equal(scratch, tops), (scratch.tolist(), tops.tolist())
        for k in (20, -20):
            s = 2.0 ** k
            scaled = _dgrad(kind, acts_dev, g_a4 * s)
            for name, a, b in zip(("g3", "g2", "gh", "g1", "scratch"), scaled, got):
                assert torch.equal(a, b * s), (name, k)


@pytest.mark.parametrize("kind", ["exact", "f16x3"])
def test_dgrad_band_seam_impulses(kind):
    """One ``g_a4`` impulse per image on either side of every 8-row band seam and at the image's top and bottom rows, first
    and last column, every mask open: what spreads over the seam (and what must not spread past the edge) against fp64."""
    dev = _dev()
    case = cc.band_seam_case()
    want = cc.dgrad_chain_ref(_dgrad_weights(), *case)
    want32 = cc.dgrad_chain_ref(_dgrad_weights(), *case, dtype=torch.float32)
    yard = [cc.max_err(a, b) for a, b in zip(want32, want)]
    yard_img = [max(cc.max_err(a[n], b[n]) for n in range(b.shape[0])) for a, b in zip(want32, want)]
    *acts_dev, g_a4 = [t.to(dev) for t in case]
    got = _dgrad(kind, acts_dev, g_a4)
    for name, a, b, y, yi in zip(("g3", "g2", "gh", "g1"), got, want, yard, yard_img):
        _held("B", f"{kind} band seams", name, cc.max_err(a, b), y)
        # image by image: an impulse's own footprint, so that one wrong row of one image is not measured against another's peak
        worst = max(cc.max_err(a[n], b[n]) for n in range(b.shape[0]))
        _held("B", f"{kind} band seams, per image", name, worst, yi)


# ============================================================================== C. ImageConvsFunction end to end
@pytest.mark.parametrize("precision", [None, "f16x3"], ids=["exact_f32", "f16x3"])
def test_image_convs_function_at_more_images_than_workgroups(precision):
    """N = C + 44: 2-3 half-images per weight-gradient workgroup, 2-3 bands per data-gradient workgroup, 44 resident
    workgroups with a second image -- outputs and all ten gradients against fp64 autograd under the kernel's own masks."""
    from multimodalfilter_amd import engine

    N = _cus() + 44
    engine.set_image_encoder_precision(precision)
    try:
        cc.image_convs_against_fp64(N, 1.0, report=lambda name, err, y: print(
            f"IMGSCALE C {precision or 'exact_f32'} N={N} {name} {err:.2e} / {y:.2e}", flush=True))
    finally:
        engine.set_image_encoder_precision(None)


# ============================================================================== D. the resident training forward
@pytest.mark.parametrize("precision", ["f16x3", "bf16"])
def test_resident_training_forward_streams_images_like_single_ones(precision):
    """N = 2 C + 44: every workgroup streams 2-3 images through the parity-selected planes while it writes the kept
    activations.  Each of ``a1, h, a2, a3, a4`` equals bit for bit the same call on slices of 100 images (one image per
    workgroup, the regime the other tests hold to fp64); f16x3: the images at the hand-overs against fp64 as well."""
    from multimodalfilter_amd import _abi, engine

    dev = _dev()
    C = _cus()
    N = 2 * C + 44
    seq = _encoder()
    blob = engine.packed_image_encoder(seq).blob()
    gen = torch.Generator().manual_seed(77)
    img = (torch.randn((N, 32, 32), generator=gen) * 0.5).clamp(-1, 1)
    imgd = img.to(dev)
    code = _abi.IMAGE_PRECISIONS[precision]

    def run(x):
        n = x.shape[0]
        outs = [_nan(n, c, 32, 32) for c in (32, 32, 32, 16, 8)]
        _abi.image_convs_train_forward(blob, x.contiguous(), *outs, engine.range_flag(dev), code)
        return outs

    big = run(imgd)
    assert not any(torch.isnan(t).any() for t in big)
    for lo in range(0, N, 100):
        for name, a, b in zip(("a1", "h", "a2", "a3", "a4"), run(imgd[lo:lo + 100]), big):
            assert torch.equal(a, b[lo:lo + 100]), (name, lo)
    if precision == "f16x3":
        rows = sorted({0, C - 1, C, 2 * C - 1, 2 * C, N - 1})
        params = cc.encoder_params(seq)
        want = cc.convs_forward_ref(params, img[rows])
        yard = [cc.max_err(a, b) for a, b in zip(cc.convs_forward_ref(params, img[rows], torch.float32), want)]
        for name, a, b, y in zip(("a1", "h", "a2", "a3", "a4"), big, want, yard):
            _held("D", f"f16x3 N={N}", name, cc.max_err(a[rows], b), y)


# ============================================================================== E. encode_images across chunks
def _encoders(spans):
    from multimodalfilter_amd import layers

    torch.manual_seed(23)
    return [layers.image_encoder(64, sp).to(_dev()) for sp in spans]


def _encode_in_chunks(encs, imgd, chunk, want_sizes, slice_len, precision):
    """``encode_images`` on the whole batch with ``_IMAGE_CHUNK = chunk`` ; checks the launch sequences'
    sizes and every row against the row of a call on at most ``slice_len`` images."""
    from multimodalfilter_amd import _abi, engine

    real, old = _abi.image_encoder, engine._IMAGE_CHUNK
    sizes = []
    engine.set_image_encoder_precision(precision)
    try:
        engine._IMAGE_CHUNK = chunk
        _abi.image_encoder = lambda blobs, images, *a: (sizes.append(images.shape[0]), real(blobs, images, *a))[1]
        big = engine.encode_images(encs, imgd)
        _abi.image_encoder = real
        n_groups = len({e[5].weight.shape[0] for e in encs})   # one launch sequence per chunk and architecture
        assert sizes == want_sizes * n_groups, sizes
        N = imgd.shape[0]
        for lo in range(0, N, slice_len):
            part = engine.encode_images(encs, imgd[lo:lo + slice_len].contiguous())
            for k, (a, b) in enumerate(zip(part, big)):
                assert torch.equal(a, b[lo:lo + slice_len]), (k, lo)
    finally:
        _abi.image_encoder = real
        engine._IMAGE_CHUNK = old
        engine.set_image_encoder_precision(None)
    return big


def _against_torch(encs, img, big, rows, precision, case):
    from multimodalfilter_amd import layers

    for k, (e, got) in enumerate(zip(encs, big)):
        twin = layers.image_encoder(64, e[5].weight.shape[0] == 2)   # the fp32 torch module on the host
        twin.load_state_dict({name: t.cpu() for name, t in e.state_dict().items()})
        with torch.no_grad():
            want = twin(img[rows][:, None])
        err = cc.max_err(got[rows], want)
        print(f"IMGSCALE E {case} encoder {k} features {err:.2e} / -", flush=True)
        assert err < (3e-2 if precision == "bf16" else 1e-4), (case, k, err)


CHUNKED = [(N, sizes, spans, precision) for N, sizes in [(257, [256, 1]), (600, [256, 256, 88])]
           for spans in [(False,), (False, False, False)] for precision in ("f32", "f16x3", "bf16")]
CHUNKED.append((600, [256, 256, 88], (False, True, False), "f16x3"))   # a spanning-pool encoder between default ones


@pytest.mark.parametrize("N,sizes,spans,precision", CHUNKED,
                         ids=[f"N{N}_{len(sp)}nets{'_mixed' if any(sp) else ''}_{pr}" for N, _, sp, pr in CHUNKED])
def test_encode_images_rows_do_not_depend_on_the_chunking(N, sizes, spans, precision):
    """With the chunk set to 256, 257 and 600 images run as 256 + 1 and 256 + 256 + 88 (several images per workgroup with
    three networks) and are concatenated per network: every row equals bit for bit the row of a call on at most 37 images,
    in every precision, and a sample of rows agrees with the torch module."""
    dev = _dev()
    encs = _encoders(spans)
    gen = torch.Generator().manual_seed(N)
    img = (torch.randn((N, 32, 32), generator=gen) * 0.5).clamp(-1, 1)
    big = _encode_in_chunks(encs, img.to(dev), 256, sizes, 37, precision)
    rows = sorted({0, 36, 37, 255, 256, N - 1})
    _against_torch(encs, img, big, rows, precision, f"{precision} N={N} nets={len(spans)}")


def test_encode_images_headline_chunking():
    """The default chunk: 4097 images of two encoders run as 2304 + 1793, about 18 images per workgroup; rows against calls
    on 256 images bit for bit, and the first and last row of each chunk and a few interior ones against the torch module."""
    dev = _dev()
    N = 4097
    encs = _encoders((False, False))
    gen = torch.Generator().manual_seed(N)
    img = (torch.randn((N, 32, 32), generator=gen) * 0.5).clamp(-1, 1)
    big = _encode_in_chunks(encs, img.to(dev), 4096, [2304, 1793], 256, "f16x3")
    rows = [0, 1, 127, 128, 1000, 2303, 2304, 2305, 3000, 4095, 4096]
    _against_torch(encs, img, big, rows, "f16x3", f"f16x3 N={N} nets=2")
