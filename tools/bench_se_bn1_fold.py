"""The SE / BatchNorm-1 backward of the fused MBConv node, old chain against new, on the block shapes of UDEB4 at
256 x 256, bs 32, fp32: graph-replayed launches, us per chain and per stage.

  old: ud_coldot_bn    -> ud_se_bwd_a, ud_se_bwd_b    -> ud_se_scale_bwd_bn -> ud_normbwd_apply[_mix]
  new: ud_coldot_bn_se -> ud_se_bwd_a, ud_se_bwd_b_bn ->                       ud_normbwd_apply[_mix]_se

The blocks whose project conv takes ud_pj_bwd_fused_a / _b have no dc tensor; their chains, in the same columns:

  old: ud_pj_bwd_fused_a    -> ud_se_bwd_a, ud_se_bwd_b    -> ud_pj_bwd_fused_b -> ud_normbwd_apply[_mix]
  new: ud_pj_bwd_fused_a_se -> ud_se_bwd_a, ud_se_bwd_b_bn ->                      ud_pj_bwd_fused_c[_mix]

This table is the source of mbconv._se_bn1_fold_policy and mbconv._pj_bn1_fold_policy.
    python tools/bench_se_bn1_fold.py [--bs 32] [--size 256]"""
import argparse
import collections
import sys

import torch

sys.path.insert(0, ".")
from unidefense_amd import kernels as K          # noqa: E402
from unidefense_amd import tape as T             # noqa: E402
from unidefense_amd.model.arch import build_arch          # noqa: E402


def block_shapes(size):
    """{(sf, stride, Ho, Ce, Cs, Co): [block indices]} of the backbone at size x size input"""
    arch = build_arch("efficientnet-b4", "ortho")
    H = T.conv_out_hw(size, size, arch["stem"]["k"], arch["stem"]["stride"], arch["stem"]["pad"])[0]
    out = collections.OrderedDict()
    for i, sp in enumerate(arch["blocks"]):
        Ho = T.conv_out_hw(H, H, sp.k, sp.stride, sp.pad)[0]
        out.setdefault((sp.sf_norm is not None, sp.stride, Ho, sp.cexp, sp.cse, sp.cout), []).append(i)
        H = Ho
    return out


def timed(fn, reps=10, rounds=5):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                K.reset_zero_pool()
                fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        g.replay()
        e0.record()
        for _ in range(rounds):
            g.replay()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / (rounds * reps) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N = a.bs
    tot_old = tot_new = pj_old = pj_new = 0.0
    print("block shape (sf, stride, Ho, Ce)    blocks | dot old -> new | FCs old -> new | scale_bwd | apply old -> new | chain old -> new  (us)")
    print("  (* thin project conv: dot = pass A / A with the five dots, scale_bwd = pass B, apply new = pass C)")
    for (sf, stride, Ho, Ce, Cs, Co), idx in block_shapes(a.size).items():
        HW = Ho * Ho
        name = "%-5s s%d %3d^2 Ce %4d" % ("SF" if sf else "plain", stride, Ho, Ce)
        pj = K.project_bwd_fused_ok(torch.empty(1), torch.empty(Co, Ce), HW)
        if pj and not K.project_bwd_fold_ok(torch.empty(Co, Ce), HW):
            print("%-34s %2d x   thin project conv (ud_pj_bwd_fused_a / _b), a pair the fold is not built for" % (name, len(idx)))
            continue
        mix = sf and stride == 1
        g = torch.Generator(device=dev).manual_seed(Ce + Ho)
        d = torch.randn(N, HW, Ce, generator=g, device=dev)
        dc = None if pj else torch.randn(N, HW, Ce, generator=g, device=dev)
        dp = torch.randn(N * HW, Co, generator=g, device=dev) if pj else None
        Wp = torch.randn(Co, Ce, generator=g, device=dev) / Ce ** 0.5 if pj else None
        diff = torch.randn(N, HW, Ce, generator=g, device=dev) if mix else None
        s2 = torch.randn(N, Ce, generator=g, device=dev)
        s1 = torch.randn(N, Cs, generator=g, device=dev)
        We = torch.randn(Ce, Cs, generator=g, device=dev) / Cs ** 0.5
        Wr = torch.randn(Cs, Ce, generator=g, device=dev) / Ce ** 0.5
        gamma, beta = torch.rand(Ce, generator=g, device=dev) + 0.5, torch.randn(Ce, generator=g, device=dev) * 0.1
        acc = torch.zeros(2 * Ce, dtype=torch.float64, device=dev)
        K.colstats(d.view(N * HW, Ce), acc)
        bn = K.DeferredBN(acc, Ce, N * HW, gamma, beta, 1e-3, 1)
        pool = torch.zeros(N * Ce, dtype=torch.float64, device=dev)
        K.colsum_bn(d, bn, N, HW, pool)
        st = {}

        def dot_old():
            st["dgate"] = K.zeros64(N * Ce, d)
            K.coldot_bn(dc, d, bn, N, HW, st["dgate"])

        def dot_new():
            st["dots"] = K.zeros64(5 * N * Ce, d)
            K.coldot_bn_se(dc, d, bn, N, HW, st["dots"])

        def fc_old():
            st["dpool"] = K.se_bwd(st["dgate"], s2, s1, We, Wr, pool, 1.0 / HW)[0]

        def fc_new():
            st["sacc"] = K.zeros64(2 * Ce, d)
            st["dpool"] = K.se_bwd(st["dots"][:N * Ce], s2, s1, We, Wr, pool, 1.0 / HW, fold=(st["dots"], 1.0 / HW, st["sacc"]))[0]

        def scale_old():
            st["sacc"] = K.zeros64(2 * Ce, d)
            st["dz"] = K.se_scale_bwd_bn(dc, d, bn, s2, st["dpool"], 1.0 / HW, N, HW, st["sacc"])

        def apply_old():
            if mix:
                K.normbwd_apply_mix(d, st["dz"], bn, N, HW, st["sacc"], diff, K.zeros64(64, d), energy=K.zeros64(Ce, d))
            else:
                K.normbwd_apply(d, st["dz"], None, 1.0, bn, True, N, HW, st["sacc"])

        def apply_new():
            if mix:
                K.normbwd_apply_mix_se(d, dc, bn, s2, st["dpool"], 1.0 / HW, N, HW, st["sacc"], diff, K.zeros64(64, d),
                                       energy=K.zeros64(Ce, d))
            else:
                K.normbwd_apply_se(d, dc, bn, s2, st["dpool"], 1.0 / HW, N, HW, st["sacc"])

        if pj:          # the same stages on the thin-project kernels: dc is re-made inside the passes
            def dot_old():
                st["dgate"] = K.zeros64(N * Ce, d)
                K.project_bwd_fused_a(d, bn, s2, dp, Wp, N, HW, st["dgate"])

            def dot_new():
                st["dots"] = K.zeros64(5 * N * Ce, d)
                K.project_bwd_fused_a_se(d, bn, s2, dp, Wp, N, HW, st["dots"])

            def scale_old():
                st["sacc"] = K.zeros64(2 * Ce, d)
                st["dz"] = K.project_bwd_fused_b(d, bn, s2, st["dpool"], 1.0 / HW, dp, Wp, N, HW, st["sacc"])

            def apply_new():
                if mix:
                    K.project_bwd_fused_c_mix(d, bn, s2, st["dpool"], 1.0 / HW, dp, Wp, N, HW, st["sacc"], diff, K.zeros64(64, d),
                                              energy=K.zeros64(Ce, d))
                else:
                    K.project_bwd_fused_c(d, bn, s2, st["dpool"], 1.0 / HW, dp, Wp, N, HW, st["sacc"])

        def chain_old():
            dot_old(), fc_old(), scale_old(), apply_old()

        def chain_new():
            dot_new(), fc_new(), apply_new()

        chain_old()
        t = {"dot0": timed(dot_old), "fc0": timed(fc_old), "sc0": timed(scale_old), "ap0": timed(apply_old)}
        chain_new()
        t.update({"dot1": timed(dot_new), "fc1": timed(fc_new), "ap1": timed(apply_new)})
        # the chains twice each, alternating: the second pair is reported, the first shows the spread
        c = [(timed(chain_old), timed(chain_new)) for _ in range(2)]
        if pj:
            pj_old += len(idx) * c[1][0]
            pj_new += len(idx) * c[1][1]
        else:
            tot_old += len(idx) * c[1][0]
            tot_new += len(idx) * c[1][1]
        print("%-34s %2d x | %5.1f -> %5.1f | %5.1f -> %5.1f | %5.1f | %5.1f -> %5.1f | %6.1f -> %6.1f  (first pair %6.1f -> %6.1f)" %
              (name + (" *" if pj else ""), len(idx), t["dot0"], t["dot1"], t["fc0"], t["fc1"], t["sc0"], t["ap0"], t["ap1"], c[1][0], c[1][1], c[0][0], c[0][1]),
              flush=True)
    print("routed blocks of one step: old chains %.1f us, new chains %.1f us, difference %.1f us" % (tot_old, tot_new, tot_old - tot_new))
    print("thin-project blocks (*) of one step: old chains %.1f us, new chains %.1f us, difference %.1f us" % (pj_old, pj_new, pj_old - pj_new))


if __name__ == "__main__":
    main()
