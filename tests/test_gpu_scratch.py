"""GPU: every user of the library's device-memory pool (csrc/scratch.h, DESIGN.md "Library-owned scratch") gives, as the FIRST library call
ever made on a fresh (non-blocking) stream, bit for bit what it gives on the current stream -- its freshly allocated scratch is zeroed on the
stream that uses it -- and ops.scratch_bytes() follows: up at a stream's first use and at growth, unchanged by repeats.  Every call is an
ordinary, valid call; all of these kernels are deterministic by design.

Shapes: the smallest that reach each pool, checked against the dispatch code (256 compute units):
  split-K forward   fp32, x [1,8,8,512], w [64,1,1,512]: M = 64, Cout = 64 -> t64 = 1 tile, nk = 512 / 32 = 16 k-tiles: dispatch_igemm's all-tiles
                    split (Cout <= 128, 2 t64 <= CUs, nk >= 16), sp = min(nk / 4, 2 CUs / t64) = 4 -> launch() asks for SCRATCH_SPLIT
  split-M wgrad     fp32, x, gy [1,32,32,64], 1x1: M = 1024 = 32 stages, one 128x128 tile, max_splits = (32 + 7) / 8 = 4, and the balance rule
                    takes all 4 (a lone workgroup on 256 CUs) -> wgrad_plan_reduction asks for SCRATCH_WGRAD
  Winograd          fp32, [1,8,8,128] with a [128,3,3,128] weight, stride 1, pad 1: conv_route's wide3x3 (Cin >= ABR_WINOGRAD_MIN_C = 128,
                    Cout >= 128), forward (V, M, and U: w_version = 0) and weight gradient (V, Mg, dU) both in SCRATCH_WINO
  bias_grad         [512,64]: grid (1, 2) -> det_ws(128 floats) and the 64 tickets of SCRATCH_BIAS_TICKETS
  smooth_l1         4096 elements: det_ws -> SCRATCH_DET
  topk_sigmoid      one image of 1024 x 2 logits, k = 64 -> SCRATCH_TOPK
  conv_prepare_batch  f16x3; the 3x3 128-wide entry packs straight from w (PrepPlan::derived: Cin % 64 == 0) and alone would travel by value, so
                    two 3x3 160-wide entries stand beside it: Cin % 64 != 0 sends them through an fp32 U (SCRATCH_PREP_U), and two jobs of a
                    kind go through the job table (SCRATCH_PREP_RING)"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _users(ops, wino_hw=8):
    """name -> (make inputs on the current stream, run(inputs) -> tuple of tensors)"""
    def split_k():
        return torch.randn(1, 8, 8, 512, device="cuda"), torch.randn(64, 1, 1, 512, device="cuda") * 0.05

    def split_m():
        return torch.randn(1, 32, 32, 64, device="cuda"), torch.randn(1, 32, 32, 64, device="cuda")

    def wino():
        return (torch.randn(1, wino_hw, wino_hw, 128, device="cuda"), torch.randn(128, 3, 3, 128, device="cuda") * 0.05,
                torch.randn(1, wino_hw, wino_hw, 128, device="cuda"))

    def run_wino(a):
        x, w, gy = a
        return ops.conv_forward(x, w, 1, 1), ops.conv_wgrad(x, gy, torch.zeros_like(w), 1, 1)

    def prep():
        return ([torch.randn(128, 3, 3, c, device="cuda") * 0.05 for c in (128, 160, 160)],
                [torch.randn(1, 8, 8, c, device="cuda") for c in (128, 160, 160)])

    def run_prep(a):
        # fresh tensors and versions every time: the derived-weight cache must not answer for the preparation
        ws = [w.clone() for w in a[0]]
        run_prep.version += 1
        ops.conv_prepare_batch([(w, None, None, 1, 1, ops.MATH_F16X3, run_prep.version) for w in ws])
        out = tuple(ops.conv_forward(x, w, 1, 1, math=ops.MATH_F16X3, w_version=run_prep.version) for x, w in zip(a[1], ws))
        run_prep.keep.append(ws)
        return out
    run_prep.version, run_prep.keep = 7000, []

    def run_smooth_l1(a):
        loss, grad = ops.smooth_l1(a[0], a[1], 1.0 / 9, want_grad=True)
        return loss[:1], grad   # (the kernel writes the first of the four floats ops.smooth_l1 hands it)

    return {
        "split_k": (split_k, lambda a: (ops.conv_forward(a[0], a[1], 1, 0),)),
        "split_m": (split_m, lambda a: (ops.conv_wgrad(a[0], a[1], torch.zeros(64, 1, 1, 64, device="cuda"), 1, 0),)),
        "winograd": (wino, run_wino),
        "bias_grad": (lambda: (torch.randn(512, 64, device="cuda"),), lambda a: (ops.bias_grad(a[0], torch.zeros(64, device="cuda")),)),
        "smooth_l1": (lambda: (torch.randn(4096, device="cuda"), torch.randn(4096, device="cuda")), run_smooth_l1),
        "topk_sigmoid": (lambda: (torch.randn(1, 1024, 2, device="cuda"),), lambda a: ops.topk_sigmoid(a[0], 2, 64)),
        "conv_prepare_batch": (prep, run_prep),
    }


def _on(stream, run, inputs):
    cur = torch.cuda.current_stream()
    stream.wait_stream(cur)
    with torch.cuda.stream(stream):
        out = run(inputs)
    cur.wait_stream(stream)
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


def test_first_call_on_a_fresh_stream_equals_the_current_stream():
    from abr_iod_amd import ops
    torch.manual_seed(0)
    users = _users(ops)
    inputs, main, side, streams = {}, {}, {}, {}
    for name, (make, run) in users.items():
        inputs[name] = make()
        main[name] = run(inputs[name])
        streams[name] = torch.cuda.Stream()          # nothing of the library has run on it
        before = ops.scratch_bytes()
        side[name] = _on(streams[name], run, inputs[name])
        assert ops.scratch_bytes() > before, name    # its first use allocated that stream's scratch
        assert _same(main[name], side[name]), name
    # repeats fit: nothing is allocated, and the results stay
    held = ops.scratch_bytes()
    for name, (make, run) in users.items():
        assert _same(run(inputs[name]), main[name]), name
        assert _same(_on(streams[name], run, inputs[name]), main[name]), name
    assert ops.scratch_bytes() == held
    # growth: the doubled Winograd shape on the side stream
    make, run = _users(ops, wino_hw=16)["winograd"]
    big = make()
    want = run(big)
    held = ops.scratch_bytes()
    got = _on(streams["winograd"], run, big)
    assert ops.scratch_bytes() > held
    assert _same(got, want)
    torch.cuda.synchronize()
