"""Certifies, without a GPU, what ``test_gpu_image_encoder_scale.py`` runs the image encoder's training kernels on
(``_conv_cases.py``): that the fp64 references are the derivatives torch autograd gives through ``layers.image_encoder``, that every impulse
case's stated answer is what the contraction of its inputs gives, and that ``engine._image_chunks`` keeps the equal-chunks
rule of ``encode_images``."""
import pytest
import torch

import _conv_cases as cc


def test_references_are_torch_autograd_through_the_encoder():
    """``convs_forward_ref``, ``dgrad_chain_ref``, ``wgrad_ref`` and ``bgrad_ref`` chained by hand against fp64 autograd
    through the module's own convolution stack, N = 2."""
    from multimodalfilter_amd import layers

    torch.manual_seed(3)
    seq = layers.image_encoder(64).double()
    params = cc.encoder_params(seq)
    gen = torch.Generator().manual_seed(4)
    img = (torch.randn((2, 32, 32), generator=gen, dtype=torch.float64) * 0.5).clamp(-1, 1)
    gout = torch.randn((2, 8, 32, 32), generator=gen, dtype=torch.float64)

    with torch.no_grad():
        a1, h, a2, a3, a4 = cc.convs_forward_ref(params, img)
    x = img[:, None]
    out = x
    for layer in list(seq)[:6]:
        out = layer(out)
    assert torch.equal(out.detach(), a4)
    assert min(float(t.max()) for t in (a1, h, a2, a3)) > 0 and min(float((t == 0).double().mean()) for t in (a1, h, a2, a3)) > 0.05
    want = torch.autograd.grad(out, params, gout)

    w1, w2a, w2b, w3, w4 = params[:5]
    with torch.no_grad():
        g3, g2, gh, g1 = cc.dgrad_chain_ref((w2a, w2b, w3, w4), a1, h, a2, a3, gout)
        got = [cc.wgrad_ref(g1, x, 5), cc.wgrad_ref(gh, a1, 3), cc.wgrad_ref(g2, h, 3), cc.wgrad_ref(g3, a2, 3),
               cc.wgrad_ref(gout, a3, 3)] + [cc.bgrad_ref(t) for t in (g1, gh, g2, g3, gout)]
    for name, a, b in zip("w1 w2a w2b w3 w4 b1 b2a b2b b3 b4".split(), got, want):
        assert a.shape == b.shape
        assert cc.max_err(a, b) < 1e-12, name


LAYERS = [(co, ci, 3) for co, ci in cc.WGRAD_LAYERS] + [(32, 1, 5)]


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("co,ci,k", LAYERS)
def test_impulse_cases_state_what_the_contraction_gives(N, co, ci, k):
    """The stated ``dW`` / ``db`` of every batch equal ``wgrad_ref`` / ``bgrad_ref`` of its inputs EXACTLY; every case's own
    cell holds 2.25 at its own tap and nothing else (or nothing at all where the case is adjacent in memory only); every case
    is placed in some batch; in fp32 the inputs and answers are exact too."""
    r = k // 2
    cases = cc.impulse_cases(N, k)
    seen = set()
    for b in cc.impulse_batches(N, co, ci, k):
        assert torch.equal(cc.wgrad_ref(b.g, b.act, k), b.dw)
        assert torch.equal(cc.bgrad_ref(b.g), b.db)
        assert torch.equal(cc.wgrad_ref(b.g, b.act, k, torch.float32).double(), b.dw)
        assert len({o for _, o, _ in b.owners}) == len(b.owners)
        if ci > 1:
            assert len({i for _, _, i in b.owners}) == len(b.owners)
        for c, o, i in b.owners:
            seen.add(c)
            assert b.g[c.gn, o, c.gy, c.gx] == cc.G_IMPULSE
            if ci > 1:
                own = torch.zeros((k, k), dtype=torch.float64)
                if c.adjacent:
                    own[c.ay - c.gy + r, c.ax - c.gx + r] = cc.DW_IMPULSE
                assert torch.equal(b.dw[o, i], own), c
                i_act = (i + 1) % ci if c.adjacent is None else i
                assert b.act[c.an, i_act, c.ay, c.ax] == cc.ACT_IMPULSE
            else:   # the stem's cases share the one input channel: the cell holds what every activation of the batch
                # within reach of this case's g makes of it, counted here from the activation tensor itself
                own = torch.zeros((k, k), dtype=torch.float64)
                for ty in range(k):
                    for tx in range(k):
                        y, x = c.gy + ty - r, c.gx + tx - r
                        if 0 <= y < 32 and 0 <= x < 32:
                            own[ty, tx] = cc.G_IMPULSE * float(b.act[c.gn, 0, y, x])
                assert torch.equal(b.dw[o, 0], own), c
                if c.adjacent:
                    assert own[c.ay - c.gy + r, c.ax - c.gx + r] >= cc.DW_IMPULSE
    skipped = set(cases) - seen
    assert all(c.adjacent is None for c in skipped)
    if ci > 1:
        assert any(c.adjacent is None for c in seen)
    else:
        assert not any(c.adjacent is None for c in seen)


def test_impulse_cases_cover_the_positions_the_kernels_split_at():
    for N in (1, 3):
        cases = cc.impulse_cases(N)
        adj = [c for c in cases if c.adjacent]
        for y, x in [(0, 0), (0, 31), (31, 0), (31, 31)] + [(y, x) for y in (15, 16) for x in (7, 8, 15, 16, 23, 24)]:
            offs = {(c.ay - y, c.ax - x) for c in adj if (c.gy, c.gx) == (y, x)}
            want = {(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if 0 <= y + dy < 32 and 0 <= x + dx < 32}
            assert offs == want, (y, x)
        assert {c.gn for c in adj} == set(range(N))
        far = [c for c in cases if not c.adjacent]
        flat = lambda n, y, x: (n * 32 + y) * 32 + x
        assert all(abs(c.ay - c.gy) > 1 or abs(c.ax - c.gx) > 1 or c.an != c.gn or c.adjacent is None for c in far)
        assert any(c.adjacent is False and c.an == c.gn and flat(0, c.ay, c.ax) - flat(0, c.gy, c.gx) == 1 for c in far)
        assert any(c.adjacent is False and c.an == c.gn and flat(0, c.ay, c.ax) - flat(0, c.gy, c.gx) == -1 for c in far)
        assert any(c.adjacent is None and (c.gy, c.ay) == (31, 0) for c in far)
        if N > 1:
            assert any(c.an == c.gn + 1 and (c.gy, c.gx, c.ay, c.ax) == (31, 31, 0, 0) for c in far)
    assert {(c.ay - c.gy, c.ax - c.gx) for c in cc.impulse_cases(1, 5) if c.adjacent and (c.gy, c.gx) == (15, 16)} == \
        {(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3)}


def test_band_seam_and_dense_inputs():
    a1, h, a2, a3, g_a4 = cc.band_seam_case()
    assert all(bool((t == 1).all()) for t in (a1, h, a2, a3))
    hits = g_a4.nonzero().tolist()
    assert len(hits) == g_a4.shape[0] == 16 and {(y, x) for _, _, y, x in hits} == {(y, x) for y in cc.SEAM_YS for x in cc.SEAM_XS}
    g, act, dw, db, y_dw, y_db = cc.dense_wgrad_case(3, 32, 32, 3)
    assert float(act.min()) == 0.0 and dw.dtype == torch.float64
    assert 0 < y_dw < 1e-5 and y_db < 1e-5      # the fp32 yardstick is far below the 1e-4 floor: the floor is the bar
    assert cc.bar(y_dw) == 1e-4 and cc.bar(1e-3) == 3e-3


@pytest.mark.parametrize("chunk", [256, 4096])
def test_image_chunks_rule(chunk):
    from multimodalfilter_amd import engine

    old = engine._IMAGE_CHUNK
    engine._IMAGE_CHUNK = chunk
    try:
        for N in range(0, 3 * chunk + 1):
            sizes = engine._image_chunks(N)
            assert sum(sizes) == N and all(0 < s <= chunk for s in sizes), N
            if N <= 256:
                assert sizes == ([N] if N else []), N
            else:
                assert all(s % 256 == 0 for s in sizes[:-1]), N
                assert len(sizes) == -(-N // chunk), N            # no more launch sequences than the bound requires
                assert len(set(sizes[:-1])) <= 1 and sizes[-1] <= sizes[0], N   # equal chunks, the short one last
        if chunk == 4096:
            assert engine._image_chunks(5120) == [2560, 2560]     # the case the rule was written for
            assert engine._image_chunks(4097) == [2304, 1793]
            assert engine._image_chunks(8192) == [4096, 4096]
        else:
            assert engine._image_chunks(257) == [256, 1]
            assert engine._image_chunks(600) == [256, 256, 88]
    finally:
        engine._IMAGE_CHUNK = old
