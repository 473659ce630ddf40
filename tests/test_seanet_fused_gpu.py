"""The fused stages of the Mimi decoder at operator level, against float64 PyTorch on the CPU: ``resblock_kernel``
(csrc/seanet.hip), ``seanet_last_kernel`` (csrc/seanet_last.hip) and ``rvq_upsample_kernel`` (csrc/mimi_engine.hip) through
their test entries ``smoltts_k_seanet_resblock`` / ``smoltts_k_seanet_last`` / ``smoltts_k_rvq_upsample``.

Reference: the modules the kernel headers cite, in float64 -- y = x + conv_k1(ELU(conv_k3(ELU(x)))) (causal), ConvTranspose1d
(stride 4, kernel 8, trimmed on the right), ELU, Conv1d k3 to one channel.  A call in mid-stream is referenced over prefix + call
rows (the halo = the prefix's last two rows) and the call's rows are compared.

Tolerance of the two fused kernels: none of its own.  The same stage is built in the test from the operator entries the suite
already holds to float64 (``ops.linear`` with the W3 tiles: PRO_ELU conv k3, EPI_RESID + elu_out conv k1, the ConvTranspose as a
GEMM, the 64 -> 1 conv); with e = max|got - ref64| / max|ref64| the fused kernel must meet e_fused < 4 e_unfused + 3e-7 (the form
and constants of tests/test_gemm_b3_gpu.py for a kernel that replaces another).  Three products: e6 < e3 < 2e-5 and other bits.
The RVQ + up-sampling stage is sums and products of fp32 table rows: rel_err < 1e-6 (as test_embed).

Every case prints e_fused, e_unfused and the place of the worst element (row, row mod 32, row mod 63).

Measured on the MI355X (256 CUs), e_fused / (4 e_unfused + 3e-7), which must stay below 1:
  resnet block     worst 0.17 over T x batch x halo (e_fused 4.2e-8 .. 1.0e-7, e_unfused 3.9e-8 .. 9.5e-8); one call against two
                   with the halo carried: bit-identical in all five splits; three products e3 7.8e-7 .. 7.5e-6 (both stages)
  last stage       row sweep T = 1 .. 1445: 0.14 .. 0.26 (e_fused 2.0e-7 .. 3.4e-7, e_unfused 1.9e-7 .. 3.3e-7);
                   120 / 258 / 768 tiles (below, just above, above twice the CU count): 0.18 / 0.12 / 0.12
  rvq + upsample   rel err 9.3e-8 .. 1.8e-7 (bound 1e-6); a stream in calls of (1, 2, 3, 1) equals one call bit for bit
Sanity of these tests, on scratch builds: with ``launch_seanet_last`` forced to three products every last-stage case fails
(e_fused 4e-6 .. 5e-6 against a bound of 1.2e-6 .. 1.6e-6); with ``stream_start`` forced false every last-stage case fails too,
its worst element in a slot_pos = 0 slot.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
C3 = 128  # channels of the stage whose resnet block runs fused


@pytest.fixture(scope="module")
def E():
    from smoltts_amd import engine

    engine.load_library()
    return engine


@pytest.fixture(scope="module")
def ops(E):
    from smoltts_amd import ops

    return ops


def _err(got: torch.Tensor, ref: torch.Tensor):
    """(e = max|got - ref| / max|ref|, flat index of the worst element)."""
    d = (got.double() - ref.double()).abs()
    return float(d.max() / (ref.double().abs().max() + 1e-30)), int(d.argmax())


class _Conv:
    """One conv of the decoder in its three forms: torch weights (float64 reference), fp32 GEMM tiles, W3 tiles."""

    def __init__(self, ops, st, key, transposed=False, stride=1):
        from smoltts_amd.packing import conv_as_gemm

        self.w, self.b = st[f"decoder.layers.{key}.conv.weight"].float(), st[f"decoder.layers.{key}.conv.bias"].float()
        self.gw, gb = conv_as_gemm(self.w, self.b, transposed, stride)
        self.N, self.K = self.gw.shape
        self.w32 = ops.pack_weight(self.gw, fp32=True)
        self.w3 = ops.pack_weight_w3(self.gw) if self.N >= 16 else None
        self.gb = gb.cuda()


@pytest.fixture(scope="module")
def weights(ops):
    """The decoder's own stage-3 block and last stage (synthetic state, seed 3): layers 9 | 11, 12, 14."""
    from smoltts_amd.codec.synthetic import synthetic_mimi_state

    st = synthetic_mimi_state(seed=3)
    return {"r2": _Conv(ops, st, "9.block.1"), "r3": _Conv(ops, st, "9.block.3"),
            "t": _Conv(ops, st, "11", True, 4), "l2": _Conv(ops, st, "12.block.1"), "l3": _Conv(ops, st, "12.block.3"),
            "f": _Conv(ops, st, "14")}


# ======================================================================================================= resnet block
def _res_ref(w, prefix: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """float64 ELU(block(prefix + x))[call rows]; prefix [B, P, C] (P = 0: the stream starts here), x [B, T, C]."""
    full = torch.cat([prefix, x], dim=1).double().transpose(1, 2)  # B, C, P + T
    h = F.conv1d(F.pad(F.elu(full), (2, 0)), w["r2"].w.double(), w["r2"].b.double())
    y = full + F.conv1d(F.elu(h), w["r3"].w.double(), w["r3"].b.double())
    return F.elu(y).transpose(1, 2)[:, prefix.shape[1]:]


def _res_buffers(x: torch.Tensor, halo: torch.Tensor, pad_rows: int):
    """xbuf [B, 2 + T + pad, C]: halo, rows, NaN behind them; out [B, 2 + T + pad, C] full of the sentinel (2 lead rows: the next
    stage's halo, which this kernel must not touch)."""
    B, T, C = x.shape
    xbuf = torch.full((B, 2 + T + pad_rows, C), float("nan"))
    xbuf[:, :2], xbuf[:, 2:2 + T] = halo, x
    out = torch.full((B, 2 + T + pad_rows, C), SENTINEL)
    return xbuf.cuda(), out.cuda()


def _res_fused(ops, w, xbuf, out, T, products=6):
    ops.seanet_resblock(xbuf, T, w["r2"].w3, w["r2"].gb, w["r3"].w3, w["r3"].gb, out, out_lead=2, b3_products=products)
    return out.cpu()


def _res_unfused(E, ops, w, xbuf, T):
    """The block as the engine runs the unfused stages: conv k3 with the ELU prologue over the halo-prefixed rows, then conv k1 +
    block input, ELU on the way out."""
    B, rows, C = xbuf.shape
    hid = torch.empty(B, T, C // 2, device="cuda")
    ops.linear(xbuf, w["r2"].w32, C // 2, w_fp32=True, prologue=E.PRO_ELU, bias=w["r2"].gb, out=hid, M=B * T, K=3 * C, ldx=C,
               x_bstride=rows * C, rows_per_batch=T, ldo=C // 2, o_bstride=T * (C // 2), elu_out=True, w3=w["r2"].w3)
    out = torch.empty(B, T, C, device="cuda")
    ops.linear(hid, w["r3"].w32, C, w_fp32=True, epilogue=E.EPI_RESID, bias=w["r3"].gb, resid=xbuf[:, 2:], ldr=C, r_bstride=rows * C,
               out=out, M=B * T, K=C // 2, ldx=C // 2, x_bstride=T * (C // 2), rows_per_batch=T, ldo=C, o_bstride=T * C, elu_out=True,
               w3=w["r3"].w3)
    return out.cpu()


def _check_untouched(buf: torch.Tensor, lead: int, T: int, what: str):
    """Everything of a sentinel-filled [B, rows, C] buffer outside rows [lead, lead + T) still holds the sentinel."""
    assert bool((buf[:, :lead] == SENTINEL).all()), f"{what}: rows in front of the output were written"
    assert bool((buf[:, lead + T:] == SENTINEL).all()), f"{what}: rows behind the output were written"


@pytest.mark.parametrize("B", [1, 3, 40])
@pytest.mark.parametrize("T", [1, 2, 31, 32, 33, 480, 481, 977])
def test_resblock_matches_float64_and_the_unfused_stage(E, ops, weights, T, B):
    """128-channel block: row counts below, at and past the 32-row tile (the ``row < T`` guards: production only ever has T = 480 F),
    stream start (zero halo) and mid-stream (random halo), slot strides larger than the rows in use with NaN behind the input
    rows and a sentinel around the output rows, both product modes."""
    g = torch.Generator().manual_seed(1000 * T + B)
    for mid in (False, True):
        x = torch.randn(B, T, C3, generator=g) * 1.5
        prefix = torch.randn(B, 7, C3, generator=g) * 1.5 if mid else torch.zeros(B, 0, C3)
        halo = prefix[:, -2:] if mid else torch.zeros(B, 2, C3)
        ref = _res_ref(weights, prefix, x)
        xbuf, out = _res_buffers(x, halo, pad_rows=3)
        got_full = _res_fused(ops, weights, xbuf, out, T)
        got = got_full[:, 2:2 + T]
        assert bool(torch.isfinite(got).all())
        _check_untouched(got_full, 2, T, f"T={T} B={B} mid={mid}")
        un = _res_unfused(E, ops, weights, xbuf, T)
        (e_f, at), (e_u, _) = _err(got, ref), _err(un, ref)
        row = at // C3 % T
        print(f"resblock T={T} B={B} {'mid-stream' if mid else 'stream start'}: e_fused {e_f:.2e}, e_unfused {e_u:.2e}, "
              f"ratio {e_f / (4 * e_u + 3e-7):.2f}; worst at slot {at // (C3 * T)} row {row} (mod 32: {row % 32}) channel {at % C3}")
        assert e_f < 4 * e_u + 3e-7
        out.fill_(SENTINEL)
        three_full = _res_fused(ops, weights, xbuf, out, T, products=3)
        three = three_full[:, 2:2 + T]
        _check_untouched(three_full, 2, T, f"T={T} B={B} mid={mid} three products")
        e3, _ = _err(three, ref)
        print(f"    three products: e3 {e3:.2e}")
        assert e_f < e3 < 2e-5 and not torch.equal(three, got)


@pytest.mark.parametrize("T1,T2", [(1, 1), (31, 2), (32, 33), (480, 1), (33, 944)])
def test_resblock_one_call_equals_two_with_the_halo_carried(E, ops, weights, T1, T2):
    """T rows in one call against T1 + T2 rows in two, the second call's halo = the first call's last two rows (what the engine's
    halo shift does): both within the bound of float64; whether the bits agree is printed, not required."""
    B, T = 3, T1 + T2
    g = torch.Generator().manual_seed(T1 * 7 + T2)
    x = torch.randn(B, T, C3, generator=g) * 1.5
    ref = _res_ref(weights, torch.zeros(B, 0, C3), x)
    xbuf, out = _res_buffers(x, torch.zeros(B, 2, C3), pad_rows=1)
    one = _res_fused(ops, weights, xbuf, out, T)[:, 2:2 + T]
    un = _res_unfused(E, ops, weights, xbuf, T)
    xa, oa = _res_buffers(x[:, :T1], torch.zeros(B, 2, C3), pad_rows=2)
    first = _res_fused(ops, weights, xa, oa, T1)[:, 2:2 + T1]
    carried = torch.cat([torch.zeros(B, 2, C3), x[:, :T1]], dim=1)[:, -2:]
    xb, ob = _res_buffers(x[:, T1:], carried, pad_rows=2)
    second = _res_fused(ops, weights, xb, ob, T2)[:, 2:2 + T2]
    two = torch.cat([first, second], dim=1)
    (e1, _), (e2, at), (e_u, _) = _err(one, ref), _err(two, ref), _err(un, ref)
    print(f"resblock {T1} + {T2} rows: one call {e1:.2e}, two calls {e2:.2e} (worst row {at // C3 % T}), unfused {e_u:.2e}; "
          f"bit-identical: {torch.equal(one, two)}")
    assert e1 < 4 * e_u + 3e-7 and e2 < 4 * e_u + 3e-7


# ========================================================================================================= last stage
PREFIX = 3  # rows of a mid-stream slot's history in the reference (the kernel sees the last two as its halo)


def _last_ref(w, inp: torch.Tensor, prefix: torch.Tensor, started: list) -> torch.Tensor:
    """float64 PCM [B, 4 T] of the call rows ``inp`` [B, T, 128] (= ELU of the stage before); slot b's stream starts with this
    call where ``started[b]``, else continues ``prefix[b]`` [PREFIX, 128]."""
    outs = []
    for b in range(inp.shape[0]):
        rows = inp[b] if started[b] else torch.cat([prefix[b], inp[b]], dim=0)
        xin = rows.double().T[None]  # 1, 128, R
        x = F.conv_transpose1d(xin, w["t"].w.double(), w["t"].b.double(), stride=4)
        x = x[..., : x.shape[-1] - 4]
        h = F.conv1d(F.pad(F.elu(x), (2, 0)), w["l2"].w.double(), w["l2"].b.double())
        y = x + F.conv1d(F.elu(h), w["l3"].w.double(), w["l3"].b.double())
        pcm = F.conv1d(F.pad(F.elu(y), (2, 0)), w["f"].w.double(), w["f"].b.double())[0, 0]
        outs.append(pcm[-4 * inp.shape[1]:])
    return torch.stack(outs)


def _last_inputs(g, B: int, T: int, pad_rows: int = 2):
    """Mixed slots: every third stream starts with this call (slot_pos 0, zero halo), the others are in mid-stream (non-zero
    position, their history's last two rows as halo).  Rows behind the T in use hold NaN."""
    inp = F.elu(torch.randn(B, T, 128, generator=g) * 1.5)
    prefix = F.elu(torch.randn(B, PREFIX, 128, generator=g) * 1.5)
    started = [b % 3 == 0 for b in range(B)]
    buf = torch.full((B, 2 + T + pad_rows, 128), float("nan"))
    buf[:, 2:2 + T] = inp
    for b in range(B):
        buf[b, :2] = 0.0 if started[b] else prefix[b, -2:]
    pos = torch.tensor([0 if started[b] else 480 * (b + 1) for b in range(B)], dtype=torch.int32)
    return inp, prefix, started, buf.cuda(), pos.cuda()


def _last_fused(ops, w, buf, T, pos, products=6, slack=8):
    B = buf.shape[0]
    pcm = torch.full((B, 4 * T + slack), SENTINEL, device="cuda")
    ops.seanet_last(buf, T, w["t"].w3, w["t"].gb, w["l2"].w3, w["l2"].gb, w["l3"].w3, w["l3"].gb,
                    w["f"].gw.reshape(-1).contiguous().cuda(), float(w["f"].b[0]), pos, pcm, b3_products=products)
    full = pcm.cpu()
    assert bool((full[:, 4 * T:] == SENTINEL).all()), "samples behind the 4 T of a slot were written"
    assert bool(torch.isfinite(full[:, :4 * T]).all())
    return full[:, :4 * T]


def _last_unfused(E, ops, w, buf, T, started):
    """The stage as four GEMM launches.  The ConvTranspose also yields the four rows in front of the call (input row -1, from the
    halo): the block's and the output conv's causal taps reach them.  Where a stream starts they are padding, i.e. zero."""
    B, rows, _ = buf.shape
    start = torch.tensor(started, device="cuda")
    Tx = 4 * (T + 1)
    x = torch.empty(B, Tx, 64, device="cuda")  # rows -4 .. 4 T - 1, raw
    ops.linear(buf, w["t"].w32, 256, w_fp32=True, bias=w["t"].gb, out=x, M=B * (T + 1), K=256, ldx=128, x_bstride=rows * 128,
               rows_per_batch=T + 1, ldo=256, o_bstride=Tx * 64, w3=w["t"].w3)
    x[start, :4] = 0.0
    Th = Tx - 2  # rows -2 .. 4 T - 1
    hid = torch.empty(B, Th, 32, device="cuda")
    ops.linear(x, w["l2"].w32, 32, w_fp32=True, prologue=E.PRO_ELU, bias=w["l2"].gb, out=hid, M=B * Th, K=192, ldx=64, x_bstride=Tx * 64,
               rows_per_batch=Th, ldo=32, o_bstride=Th * 32, elu_out=True, w3=w["l2"].w3)
    y = torch.empty(B, Th, 64, device="cuda")
    ops.linear(hid, w["l3"].w32, 64, w_fp32=True, epilogue=E.EPI_RESID, bias=w["l3"].gb, resid=x[:, 2:], ldr=64, r_bstride=Tx * 64, out=y,
               M=B * Th, K=32, ldx=32, x_bstride=Th * 32, rows_per_batch=Th, ldo=64, o_bstride=Th * 64, elu_out=True, w3=w["l3"].w3)
    y[start, :2] = 0.0
    pcm = torch.empty(B, 4 * T, device="cuda")
    ops.linear(y, w["f"].w32, 1, w_fp32=True, bias=w["f"].gb, out=pcm, M=B * 4 * T, K=192, ldx=64, x_bstride=Th * 64, rows_per_batch=4 * T,
               ldo=1, o_bstride=4 * T)
    return pcm.cpu()


def _last_case(E, ops, w, B, T, label):
    g = torch.Generator().manual_seed(31 * T + B)
    inp, prefix, started, buf, pos = _last_inputs(g, B, T)
    ref = _last_ref(w, inp, prefix, started)
    got = _last_fused(ops, w, buf, T, pos)
    un = _last_unfused(E, ops, w, buf, T, started)
    (e_f, at), (e_u, _) = _err(got, ref), _err(un, ref)
    slot, row = at // (4 * T), at % (4 * T) // 4
    tiles = B * ((T + 62) // 63)
    print(f"last stage {label}: B={B} T={T} ({tiles} tiles): e_fused {e_f:.2e}, e_unfused {e_u:.2e}, ratio {e_f / (4 * e_u + 3e-7):.2f}; "
          f"worst at slot {slot} ({'start' if started[slot] else 'mid-stream'}) row {row} (mod 32: {row % 32}, mod 63: {row % 63})")
    assert e_f < 4 * e_u + 3e-7
    # the stream's first samples on their own: the stream-start special case (zero padding, not data, in front of row 0)
    for b in range(B):
        if started[b]:
            d = float((got[b, :16].double() - ref[b, :16]).abs().max() / ref.abs().max())
            assert d < 4 * e_u + 3e-7, f"slot {b} (stream start): first samples off by {d:.2e}"
    three = _last_fused(ops, w, buf, T, pos, products=3)
    e3, _ = _err(three, ref)
    print(f"    three products: e3 {e3:.2e}")
    assert e_f < e3 < 2e-5 and not torch.equal(three, got)
    return e_f, e_u


@pytest.mark.parametrize("T", [1, 2, 62, 63, 64, 126, 127, 480, 1445])
def test_last_stage_matches_float64_and_the_unfused_stage(E, ops, weights, T):
    """128 -> 64 -> PCM: row counts below, at and just past the 63-row tile stride and the 32-row halves; three slots in one
    launch, one at its stream's start (slot_pos 0, zero halo) beside two in mid-stream; a sentinel behind the samples."""
    _last_case(E, ops, weights, 3, T, "row sweep")


def test_last_stage_persistent_rounds(E, ops, weights):
    """Tile counts below the CU count, just above it and above twice it: the persistent loop and the register prefetch of the next
    tile run once, twice (for some workgroups) and three times per workgroup."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    below = max(1, n_cu // 16 - 1)             # x 8 tiles (T = 480) < n_cu
    just_above = n_cu // 2 + 1                 # x 2 tiles (T = 126) = n_cu + 2
    twice = max(48, (2 * n_cu) // 16 + 2)      # x 16 tiles (T = 960) > 2 n_cu  (48 x 16 = 768 on 256 CUs)
    assert below * 8 < n_cu < just_above * 2 <= n_cu + 2 and twice * 16 > 2 * n_cu
    print(f"{n_cu} CUs")
    _last_case(E, ops, weights, below, 480, "below the CU count")
    _last_case(E, ops, weights, just_above, 126, "just above the CU count")
    _last_case(E, ops, weights, twice, 960, "above twice the CU count")


# ================================================================================================== RVQ + up-sampling
@pytest.fixture(scope="module")
def rvq(ops):
    from oracle.mimi_oracle import MimiDecodeOracle
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.packing import pack_mimi

    st = synthetic_mimi_state(seed=3)
    arena, off = pack_mimi(st, 8, max_positions=64)
    t0, u0 = off["rvq_table"], off["upsample_w"]
    table = arena[t0: t0 + 8 * 2048 * 512 * 4].view(torch.float32).view(8, 2048, 512).cuda()
    upw = arena[u0: u0 + 4 * 512 * 4].view(torch.float32).view(4, 512).cuda()
    return MimiDecodeOracle(st, dtype=torch.float64), table, upw


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


@pytest.mark.parametrize("Fr", [1, 2, 7])
@pytest.mark.parametrize("code_offset", [0, 1])
def test_rvq_upsample_matches_float64(ops, rvq, Fr, code_offset):
    """One call from a stream's start (zero carry) against ``intermediates()["upsample"]`` of the float64 oracle; code_offset = 1
    reads the codes out of wider rows ([slow id, c0 .. c7, spare]) whose other columns hold out-of-range values."""
    orc, table, upw = rvq
    B, row = 3, 8 + 2 * code_offset
    g = torch.Generator().manual_seed(10 * Fr + code_offset)
    codes = torch.randint(0, 2048, (B, Fr, 8), generator=g)
    grid = torch.full((B, Fr + 1, row), 1 << 20, dtype=torch.int32)  # (one spare frame behind the call's)
    grid[:, :Fr, code_offset:code_offset + 8] = codes.int()
    ref = orc.intermediates(codes.permute(0, 2, 1))["upsample"]
    carry_in, carry_out = torch.zeros(B, 512, device="cuda"), torch.full((B, 512), SENTINEL, device="cuda")
    tx = ops.rvq_upsample(grid.cuda(), 0, Fr, 8, table, upw, carry_in, carry_out, code_offset=code_offset).cpu()
    e = _rel(tx, ref)
    print(f"rvq + upsample F={Fr} code_offset={code_offset}: rel err {e:.2e}")
    assert tx.shape == ref.shape and e < 1e-6
    e_last = orc.intermediates(codes.permute(0, 2, 1))["rvq"][:, -1]
    assert _rel(carry_out.cpu(), e_last) < 1e-6  # the carry = the last frame's embedding


def test_rvq_upsample_stream_in_calls_and_stateless(ops, rvq):
    """A stream of 7 frames cut into calls of 1, 2, 3 and 1 frames with the carry ping-ponged by the test == one call == the
    float64 oracle; ``carry_in = None`` (stateless mode): every call's first frame has no predecessor, i.e. the oracle's per-call
    up-sampling."""
    orc, table, upw = rvq
    B, Fr, plan = 2, 7, (1, 2, 3, 1)
    codes = torch.randint(0, 2048, (B, Fr, 8), generator=torch.Generator().manual_seed(77))
    dev = codes.int().cuda()
    ref = orc.intermediates(codes.permute(0, 2, 1))["upsample"]
    carry = [torch.zeros(B, 512, device="cuda"), torch.zeros(B, 512, device="cuda")]
    parts, stateless, f0 = [], [], 0
    for i, n in enumerate(plan):
        parts.append(ops.rvq_upsample(dev, f0, n, 8, table, upw, carry[i & 1], carry[(i & 1) ^ 1]).cpu())
        spare = torch.empty(B, 512, device="cuda")
        stateless.append(ops.rvq_upsample(dev, f0, n, 8, table, upw, None, spare).cpu())
        f0 += n
    got = torch.cat(parts, dim=1)
    whole = ops.rvq_upsample(dev, 0, Fr, 8, table, upw, torch.zeros(B, 512, device="cuda"), torch.empty(B, 512, device="cuda")).cpu()
    print(f"rvq + upsample in calls of {plan}: rel err {_rel(got, ref):.2e}; equal to one call: {torch.equal(got, whole)}")
    assert _rel(got, ref) < 1e-6 and _rel(whole, ref) < 1e-6
    e = orc.rvq_decode(codes.permute(0, 2, 1))
    ref_sl, f0 = [], 0
    for n in plan:
        ref_sl.append(orc.upsample(e[:, :, f0:f0 + n]).transpose(1, 2))
        f0 += n
    ref_sl = torch.cat(ref_sl, dim=1)
    assert _rel(torch.cat(stateless, dim=1), ref_sl) < 1e-6 and _rel(ref_sl, ref) > 1e-3


def test_rvq_upsample_clamps_codes(ops, rvq):
    """Codes at the table's ends (0, 2047) and out of range (-1, 2048, 1 << 20), which the kernel documents as clamped to
    [0, 2047]: equal to the float64 oracle on the clamped codes."""
    orc, table, upw = rvq
    vals = torch.tensor([0, 2047, -1, 2048, 1 << 20, 5, 2046, 1], dtype=torch.int64)
    codes = torch.stack([vals.roll(i) for i in range(6)])[None].repeat(2, 1, 1)  # [2, 6 frames, 8]
    codes[1] = codes[1].flip(-1)
    ref = orc.intermediates(codes.clamp(0, 2047).permute(0, 2, 1))["upsample"]
    tx = ops.rvq_upsample(codes.int().cuda(), 0, 6, 8, table, upw, torch.zeros(2, 512, device="cuda"), torch.empty(2, 512, device="cuda")).cpu()
    assert bool(torch.isfinite(tx).all()) and _rel(tx, ref) < 1e-6
