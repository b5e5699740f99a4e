"""Float64 restatements shared by the conv tests and the random sweep (tools/conv_fuzz.py): the one-product fp16 arithmetic's operand rounding
(ABR_MATH_F16: x ~ s q16(x / s), include/abr_iod_hip.h) and NHWC / OHWI convolution and weight gradient on the CPU."""
import torch
import torch.nn.functional as F


def q16(t, per_row=False):
    """s q16(t / s) in float64 on the CPU; per_row: one scale per output row of a [Cout, R, S, Cin] weight"""
    t64 = t.detach().double().cpu()
    a = t64.abs().flatten(1).amax(1).view(-1, *([1] * (t64.dim() - 1))) if per_row else t64.abs().max()
    _, e = torch.frexp(a)                                   # a = m 2^e, m in [0.5, 1)
    s = torch.where(a > 0, torch.exp2((e - 15).double()), torch.ones_like(a, dtype=torch.float64))
    return (t64 / s).to(torch.float16).double() * s


def conv64(x, w, stride, pad):
    """NHWC x, OHWI w (float64) -> NHWC"""
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=stride, padding=pad).permute(0, 2, 3, 1)


def wgrad64(x, gy, R, stride, pad):
    """dW[n, r, s, c] = sum_{b, ho, wo} gy[b, ho, wo, n] x[b, ho * stride - pad + r, wo * stride - pad + s, c] (NHWC, float64)"""
    Ho, Wo = gy.shape[1], gy.shape[2]
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    out = torch.zeros(gy.shape[3], R, R, x.shape[3], dtype=torch.float64)
    g2 = gy.reshape(-1, gy.shape[3])
    for r in range(R):
        for s in range(R):
            xs = xp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride, :].reshape(-1, x.shape[3])
            out[:, r, s, :] = g2.t() @ xs
    return out


# ---- what a run of tools/conv_fuzz.py must have covered (its COVERAGE line), per group of strata ------------------------------------------
FUZZ_GROUPS = {"winograd": ["wino", "wino_wgrad_only"], "reduced": ["f16", "bf16_fallback"], "fused": ["tail64", "dgrad_fused"]}
FUZZ_FULL = ["f32", "bf16x6", "f16x3"]                 # the arithmetics that may take Winograd
FUZZ_WINO_OPS = ["fwd", "dgrad", "wgrad", "wgrad_kept_v"]
FUZZ_WINO_FEATS = ["H%%4=%d" % r for r in range(4)] + ["W%%4=%d" % r for r in range(4)] + ["below_one_tile", "batch40_one_tile"]
FUZZ_OFF_ROUTE = {"residual": FUZZ_FULL, "cout_not_32_split": FUZZ_FULL[1:], "cout_not_4": FUZZ_FULL, "cin_not_32": FUZZ_FULL}


def fuzz_coverage(stdout):
    import json
    line = [ln for ln in stdout.splitlines() if ln.startswith("COVERAGE ")][-1]
    return json.loads(line[len("COVERAGE "):])


def fuzz_coverage_problems(cov, strata, per_stratum, ran=True):
    """the conditions on the sweep's generator, as a list of what is missing (empty: covered).  ran=False: a --plan run, which compares nothing"""
    bad = []

    def need(ok, what):
        if not ok:
            bad.append(what)

    for st in strata:
        c = cov.get(st)
        if c is None:
            bad.append("stratum %s did not run" % st)
            continue
        need(c["cases"] >= per_stratum, "%s: %d cases < %d" % (st, c["cases"], per_stratum))
        need(c["misrouted"] == 0, "%s: %d drawn cases the library routes elsewhere" % (st, c["misrouted"]))
        need(not ran or c["comparisons"] > 0, "%s: no comparison ran" % st)
        if ran:     # every forward / input-gradient result that was compared had its amax word read and compared with max |result| as well
            for m, n in sorted(c.get("fwd_dgrad", {}).items()):
                k = c.get("amax_checks", {}).get(m, 0)
                need(n == 0 or (k > 0 and k >= n), "%s: %s compared %d forward / input-gradient results but checked %d amax words" % (st, m, n, k))
            need("fwd_dgrad" in c and "amax_checks" in c, "%s: the run does not report its amax checks" % st)
        routes, feats = c["routes"], c["features"]
        if st == "wino":
            for m in FUZZ_FULL:
                for op in FUZZ_WINO_OPS:
                    need(routes.get(m, {}).get(op + "/wino", 0) >= 1 and routes.get(m, {}).get(op + "/direct", 0) == 0, "wino: %s %s not all Winograd" % (m, op))
                    for f in FUZZ_WINO_FEATS:
                        need(feats.get(m, {}).get(op, {}).get(f, 0) >= 1, "wino: no confirmed-Winograd %s %s with %s" % (m, op, f))
        elif st == "wino_wgrad_only":
            for reason, modes in FUZZ_OFF_ROUTE.items():
                for m in modes:
                    need(c["reasons"].get(reason, {}).get(m, 0) >= 1, "wino_wgrad_only: %s never off the forward route by %s" % (m, reason))
            for m in FUZZ_FULL:
                need(routes.get(m, {}).get("fwd/wino", 0) == 0 and routes.get(m, {}).get("wgrad/direct", 0) == 0, "wino_wgrad_only: %s on another route" % m)
        elif st == "f16":
            for op in ("fwd", "dgrad", "wgrad"):
                need(routes.get("f16", {}).get(op + "/direct", 0) >= 1, "f16: no %s in the mode" % op)
                need(routes.get("f16", {}).get(op + "/wino", 0) == 0, "f16: a Winograd %s" % op)
                need(feats.get("f16", {}).get(op, {}).get("wide3x3", 0) >= 1, "f16: no wide 3x3 %s" % op)
        elif st == "bf16_fallback":
            for op in ("fwd", "dgrad", "wgrad"):
                r = routes.get("bf16->f32", {})
                need(r.get(op + "/direct", 0) >= 1 and r.get(op + "/wino", 0) >= 1, "bf16_fallback: %s not on both fp32 routes" % op)
        elif st == "tail64":
            for f in ("one_pixel_row_or_column", "ragged_last_tile"):
                need(feats.get("bf16x6", {}).get("tail64", {}).get(f, 0) >= 1, "tail64: no case with %s" % f)
        elif st == "dgrad_fused":
            for m in FUZZ_FULL + ["bf16"]:
                for f in ("mask", "residual", "mask+residual"):
                    for sc in ("", " scattered"):
                        need(feats.get(m, {}).get("dgrad", {}).get(f + sc, 0) >= 1, "dgrad_fused: no %s %s" % (m, f + sc))
    return bad
