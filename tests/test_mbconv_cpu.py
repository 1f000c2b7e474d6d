"""CPU: the host logic of the MBConv block nodes (unidefense_amd/mbconv.py) that runs before any HIP call — the two depthwise
policies against literal tables (the rules of the fused node were moved here from tape.py: a slip while moving them shows as a
changed row), their override and kill switches, and the geometry record against the closed-form sizes."""
import math

import pytest
import torch

# per block of build_arch("efficientnet-b4", "ortho") at its map side for a 256 x 256 / 320 x 320 input:
# (block, sf, k, stride, H, _dw_tile_policy fp32 (forward, weight gradient, data gradient), _dw_bwd_fused_policy fp32,
#  _dw_tile_policy half storage, _dw_bwd_fused_policy half storage)
POLICIES = {
    256: [
        (0, False, 3, 1, 128, (True, True, False), True, (True, True, True), True),
        (1, False, 3, 1, 128, (True, True, False), True, (True, True, True), True),
        (2, False, 3, 2, 128, (True, True, True), False, (True, True, False), False),
        (3, False, 3, 1, 64, (True, True, True), False, (True, True, True), True),
        (4, False, 3, 1, 64, (True, True, True), False, (True, True, True), True),
        (5, False, 3, 1, 64, (True, True, True), False, (True, True, True), True),
        (6, True, 5, 2, 64, (True, False, True), False, (True, True, True), False),
        (7, True, 5, 1, 32, (True, False, True), True, (True, True, True), True),
        (8, True, 5, 1, 32, (True, False, True), True, (True, True, True), True),
        (9, True, 5, 1, 32, (True, False, True), True, (True, True, True), True),
        (10, True, 3, 2, 32, (False, False, True), False, (True, True, True), False),
        (11, True, 3, 1, 16, (True, False, False), True, (True, True, True), True),
        (12, True, 3, 1, 16, (True, False, False), True, (True, True, True), True),
        (13, True, 3, 1, 16, (True, False, False), True, (True, True, True), True),
        (14, True, 3, 1, 16, (True, False, False), True, (True, True, True), True),
        (15, True, 3, 1, 16, (True, False, False), True, (True, True, True), True),
        (16, True, 5, 1, 16, (True, False, True), True, (True, True, True), True),
        (17, True, 5, 1, 16, (True, False, True), True, (True, True, True), True),
        (18, True, 5, 1, 16, (True, False, True), True, (True, True, True), True),
        (19, True, 5, 1, 16, (True, False, True), True, (True, True, True), True),
        (20, True, 5, 1, 16, (True, False, True), True, (True, True, True), True),
        (21, True, 5, 1, 16, (True, False, True), True, (True, True, True), True),
        (22, True, 5, 2, 16, (False, False, True), False, (True, True, True), False),
        (23, True, 5, 1, 8, (False, False, False), False, (True, True, True), False),
        (24, True, 5, 1, 8, (False, False, False), False, (True, True, True), False),
        (25, True, 5, 1, 8, (False, False, False), False, (True, True, True), False),
        (26, True, 5, 1, 8, (False, False, False), False, (True, True, True), False),
        (27, True, 5, 1, 8, (False, False, False), False, (True, True, True), False),
        (28, True, 5, 1, 8, (False, False, False), False, (True, True, True), False),
        (29, True, 5, 1, 8, (False, False, False), False, (True, True, True), False),
        (30, False, 3, 1, 8, (True, True, False), True, (True, True, True), False),
        (31, False, 3, 1, 8, (True, True, False), True, (True, True, True), False),
    ],
    320: [
        (0, False, 3, 1, 160, (True, True, False), True, (True, True, True), True),
        (1, False, 3, 1, 160, (True, True, False), True, (True, True, True), True),
        (2, False, 3, 2, 160, (True, True, True), False, (True, True, False), False),
        (3, False, 3, 1, 80, (True, True, False), True, (True, True, True), True),
        (4, False, 3, 1, 80, (True, True, False), True, (True, True, True), True),
        (5, False, 3, 1, 80, (True, True, False), True, (True, True, True), True),
        (6, True, 5, 2, 80, (True, False, True), False, (True, True, True), False),
        (7, True, 5, 1, 40, (True, False, True), True, (True, True, True), True),
        (8, True, 5, 1, 40, (True, False, True), True, (True, True, True), True),
        (9, True, 5, 1, 40, (True, False, True), True, (True, True, True), True),
        (10, True, 3, 2, 40, (False, False, True), False, (True, True, True), False),
        (11, True, 3, 1, 20, (True, False, False), True, (True, True, True), True),
        (12, True, 3, 1, 20, (True, False, False), True, (True, True, True), True),
        (13, True, 3, 1, 20, (True, False, False), True, (True, True, True), True),
        (14, True, 3, 1, 20, (True, False, False), True, (True, True, True), True),
        (15, True, 3, 1, 20, (True, False, False), True, (True, True, True), True),
        (16, True, 5, 1, 20, (True, False, True), True, (True, True, True), True),
        (17, True, 5, 1, 20, (True, False, True), True, (True, True, True), True),
        (18, True, 5, 1, 20, (True, False, True), True, (True, True, True), True),
        (19, True, 5, 1, 20, (True, False, True), True, (True, True, True), True),
        (20, True, 5, 1, 20, (True, False, True), True, (True, True, True), True),
        (21, True, 5, 1, 20, (True, False, True), True, (True, True, True), True),
        (22, True, 5, 2, 20, (False, False, True), False, (True, True, True), False),
        (23, True, 5, 1, 10, (True, False, False), True, (True, True, True), True),
        (24, True, 5, 1, 10, (True, False, False), True, (True, True, True), True),
        (25, True, 5, 1, 10, (True, False, False), True, (True, True, True), True),
        (26, True, 5, 1, 10, (True, False, False), True, (True, True, True), True),
        (27, True, 5, 1, 10, (True, False, False), True, (True, True, True), True),
        (28, True, 5, 1, 10, (True, False, False), True, (True, True, True), True),
        (29, True, 5, 1, 10, (True, False, False), True, (True, True, True), True),
        (30, False, 3, 1, 10, (True, True, False), True, (True, True, True), True),
        (31, False, 3, 1, 10, (True, True, False), True, (True, True, True), True),
    ],
}


def _walk(size):
    """(block index, spec, map side) of every block for a size x size input"""
    from unidefense_amd import tape as T
    from unidefense_amd.model.arch import build_arch
    arch = build_arch("efficientnet-b4", "ortho")
    H = T.conv_out_hw(size, size, 3, 2, arch["stem"]["pad"])[0]
    for i, sp in enumerate(arch["blocks"]):
        yield i, sp, H
        H = T.conv_out_hw(H, H, sp.k, sp.stride, sp.pad)[0]


@pytest.mark.parametrize("size", [256, 320])
def test_depthwise_policies_match_the_recorded_tables(size):
    from unidefense_amd import mbconv as MB
    assert MB._DW_TILED and not MB._DW_TILE_OVERRIDE and not MB._DW_BWD_FUSED_OVERRIDE
    rows = POLICIES[size]
    assert len(rows) == 32
    for (i, sp, H), row in zip(_walk(size), rows):
        sf = sp.sf_norm is not None
        assert (i, sf, sp.k, sp.stride, H) == row[:5]
        for half, (tile, fused) in ((False, row[5:7]), (True, row[7:9])):
            assert tuple(MB._dw_tile_policy(sf, sp.k, sp.stride, H, half)) == tile, (i, half)
            assert MB._dw_bwd_fused_policy(sf, sp.k, sp.stride, H, half) is fused, (i, half)


def test_an_override_entry_wins(monkeypatch):
    from unidefense_amd import mbconv as MB
    key = (True, 5, 1, 32, False)
    assert tuple(MB._dw_tile_policy(*key)) == (True, False, True) and MB._dw_bwd_fused_policy(*key) is True
    monkeypatch.setitem(MB._DW_TILE_OVERRIDE, key, (False, True, False))
    monkeypatch.setitem(MB._DW_BWD_FUSED_OVERRIDE, key, False)
    assert tuple(MB._dw_tile_policy(*key)) == (False, True, False) and MB._dw_bwd_fused_policy(*key) is False
    assert tuple(MB._dw_tile_policy(1, 5, 1, 32, 0)) == (False, True, False)          # keys are normalised to bool
    assert tuple(MB._dw_tile_policy(True, 5, 1, 16, False)) == (True, False, True)     # another shape keeps the rule


def test_dw_tiled_off_switches_the_tile_policy_only(monkeypatch):
    from unidefense_amd import mbconv as MB
    monkeypatch.setitem(MB._DW_TILE_OVERRIDE, (True, 5, 1, 32, False), (True, True, True))          # ignored while off
    monkeypatch.setattr(MB, "_DW_TILED", False)
    for size, rows in POLICIES.items():
        for (i, sp, H), row in zip(_walk(size), rows):
            sf = sp.sf_norm is not None
            for half, fused in ((False, row[6]), (True, row[8])):
                assert tuple(MB._dw_tile_policy(sf, sp.k, sp.stride, H, half)) == (False, False, False)
                assert MB._dw_bwd_fused_policy(sf, sp.k, sp.stride, H, half) is fused


@pytest.mark.parametrize("size", [256, 320])
def test_block_geom_is_the_closed_form(size):
    """TF-'SAME' pads are fixed for the 380 x 380 design resolution.  Stride 1: total pad k - 1, the side is kept.  Stride 2: the four
    down-sampling blocks were padded for the sides 190, 95, 48, 24 — totals 1, 4 (an odd side: k - 1), 1, 3, the smaller half on
    top / left — and every even side H gives H / 2 with them."""
    from unidefense_amd import mbconv as MB
    from unidefense_amd.model.unidefense import _MBConvParams
    n = 2
    top_left = {2: 0, 6: 2, 10: 0, 22: 1}                                                  # the stride-2 blocks' top / left pad
    for i, sp, H in _walk(size):
        blk = _MBConvParams(sp, 1e-3, 0.01)
        g = MB.block_geom(blk, torch.empty(n, H, H, sp.cin))
        assert (sp.stride == 2) == (i in top_left) and H % sp.stride == 0
        pad = top_left[i] if sp.stride == 2 else (sp.k - 1) // 2
        Ho = math.ceil(H / sp.stride)
        assert (g.N, g.H, g.W, g.Cin, g.M) == (n, H, H, sp.cin, n * H * H)
        assert (g.k, g.stride, g.Ce, g.Co, g.Cs) == (sp.k, sp.stride, sp.cexp, sp.cout, sp.cse)
        assert (g.Ho, g.Wo, g.HWo, g.Mo) == (Ho, Ho, Ho * Ho, n * Ho * Ho), (i, H)
        assert (g.pt, g.pl) == (pad, pad)
        assert (g.We is None) == (sp.expand == 1) and (g.We is None or g.We.shape == (sp.cexp, sp.cin))
        assert g.Wsr.shape == (sp.cse, sp.cexp) and g.Wse.shape == (sp.cexp, sp.cse) and g.Wp.shape == (sp.cout, sp.cexp)
        assert g.Wp.data_ptr() == blk._project_conv.weight.data_ptr()                      # views, not copies
        assert g.sf == (sp.sf_norm is not None)
        if g.sf:
            assert g.Wf.shape == (2 * sp.cexp, 2 * sp.cexp) and g.alpha is blk._depthwise_conv.sf_coef
            assert (g.s_f, g.s_i) == (1.0 / H, 1.0 / H)                                    # "ortho"
        else:
            assert g.Wf is None and g.alpha is None and g.s_f is None and g.s_i is None
    with pytest.raises(AttributeError):
        g.Ho = 1                                                                           # immutable


def test_block_geom_odd_side_and_asymmetric_pad():
    """a stride-2 block on an odd side with the pad halves apart (top / left 1, bottom / right 2): floor((H + 3 - k) / 2) + 1"""
    from unidefense_amd import mbconv as MB
    from unidefense_amd.model.arch import BlockSpec
    from unidefense_amd.model.unidefense import _MBConvParams
    sp = BlockSpec(cin=8, cout=16, cexp=48, expand=6, k=5, stride=2, pad=(1, 2, 1, 2), cse=2, sf_norm=None, skip=False)
    g = MB.block_geom(_MBConvParams(sp, 1e-3, 0.01), torch.empty(3, 15, 11, 8))
    assert (g.Ho, g.Wo, g.HWo, g.Mo, g.M, g.pt, g.pl) == (7, 5, 35, 105, 3 * 15 * 11, 1, 1)


def test_block_geom_takes_the_weight_views_per_call():
    from unidefense_amd import mbconv as MB
    from unidefense_amd.model.arch import build_arch
    from unidefense_amd.model.unidefense import _MBConvParams
    sp = build_arch("efficientnet-b4", "backward")["blocks"][7]
    blk = _MBConvParams(sp, 1e-3, 0.01)
    x = torch.empty(1, 32, 32, sp.cin)
    g0 = MB.block_geom(blk, x)
    assert (g0.s_f, g0.s_i) == (1.0, 1.0 / (32 * 32))
    blk._project_conv.weight = torch.nn.Parameter(torch.zeros_like(blk._project_conv.weight))          # what .to() does
    assert MB.block_geom(blk, x).Wp.data_ptr() == blk._project_conv.weight.data_ptr() != g0.Wp.data_ptr()
