"""quantized_maxrelu / quantized_leakymaxrelu without a GPU: the contract (include/qnn_abi_maxact.h, restated in
maxrelu_cases.py) against the reference's own vectors, the band where the reference depends on its float32 log, the
degenerate inputs, the maximum of a sharded batch over two gloo ranks, and the Python surface."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import qnn_amd
from qnn_amd import _abi, engine, nets, shard
import maxrelu_cases as C

quantized_ops = engine.quantized_ops
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.mark.parametrize("nb", C.NBS)
def test_the_contract_equals_the_reference_vectors_bit_for_bit(nb):
    for ci, M in enumerate(C.MAXIMA):
        x, mx, lk = C.fixture(nb, ci)
        assert x.size > 2000 and x.max() == M and mx.shape == lk.shape == x.shape
        assert C.same_bits(C.maxact(x, nb, "quantized_maxrelu"), mx), (nb, float(M))
        assert C.same_bits(C.maxact(x, nb, "quantized_leakymaxrelu"), lk), (nb, float(M))
        # max L(x) = max r(x) whenever a value is positive
        assert C.leaky(x).max() == C.batch_max(x) == M


@pytest.mark.parametrize("nb", C.NBS)
def test_the_vectors_hold_the_points_the_contract_turns_on(nb):
    m = 2.0 ** (nb - 1)
    for ci, M in enumerate(C.MAXIMA):
        x, mx, lk = C.fixture(nb, ci)
        e = C.scale_exponent(M)
        P = 2.0 ** e
        assert P / 2 < M < P                      # far from a power of two: every log agrees on the ceiling
        step = P / m
        have = set(x.view(np.int32).tolist())

        def has(v):
            return int(np.asarray(v, dtype=F32).view(np.int32)) in have
        for j in range(int(-m) - 1, int(m) + 1):
            for t in ((j + 0.5) * step,) + ((10.0 * (j + 0.5) * step,) if j < 0 else ()):
                for c in (F32(t), np.nextafter(F32(t), F32(-np.inf)), np.nextafter(F32(t), F32(np.inf))):
                    assert has(c) or c > M, (nb, float(M), j, t)
        assert has(0.0) and has(-0.0) and has(M)
        for edge in ((m - 1) * step, -m * step, -10.0 * m * step):
            for c in (np.nextafter(F32(edge), F32(-np.inf)), np.nextafter(F32(edge), F32(np.inf))):
                assert has(c) or c > M, edge             # (a maximum below the upper clip edge never reaches it)
        assert x.min() < -1.49 * M
        # both grids are reached end to end, on the scale P / m; a zero is +0
        top = int(np.floor(M / step + 0.5))
        assert set(np.unique(mx / F32(step)).tolist()) == set(range(0, min(top, int(m) - 1) + 1))
        assert lk.min() == F32(-P) and set(np.unique(lk / F32(step)).tolist()) >= set(range(int(-m), min(top, int(m) - 1) + 1))
        assert not np.signbit(mx[mx == 0]).any() and not np.signbit(lk[lk == 0]).any()


def test_the_ambiguous_band_is_the_exact_scale_or_one_binade_off(capsys):
    """M = 2^k and up to 16 ulp above it: the reference's ceil(log(M) / log(2)) may be one off, depending on its float32
    log.  The recorded answers are the contract's, or the contract's with the scale doubled or halved -- nothing else."""
    count = {0: 0, 1: 0, -1: 0}
    for i, M in enumerate(C.AMBIGUOUS):
        for nb in C.NBS:
            x, mx, lk = C.fixture_ambiguous(nb, i)
            assert x[0] == M == x.max()
            for fn, rec in (("quantized_maxrelu", mx), ("quantized_leakymaxrelu", lk)):
                hit = [s for s in (0, 1, -1) if C.same_bits(C.maxact(x, nb, fn, shift=s), rec)]
                assert hit, (float(M), nb, fn)
                count[hit[0]] += 1
    with capsys.disabled():
        print("\nambiguous band, recorded reference answers: %d at the exact scale, %d at twice, %d at half of it"
              % (count[0], count[1], count[-1]))
    assert sum(count.values()) == len(C.AMBIGUOUS) * len(C.NBS) * 2 and count[0] > 0
    # the exact rule itself: P = M at a power of two, 2 M one ulp above it
    for k in (-15, 0, 13):
        assert C.scale_exponent(F32(2.0 ** k)) == k and C.scale_exponent(np.nextafter(F32(2.0 ** k), F32(np.inf))) == k + 1
        assert C.scale_exponent(np.nextafter(F32(2.0 ** k), F32(0))) == k


def test_degenerate_and_out_of_range_maxima_give_nan_everywhere():
    for fn in C.FNS:
        for x in (np.zeros(7, F32), -np.ones(7, F32), np.array([-0.0, -3.0], F32),
                  np.array([2.0 ** -65, -1.0], F32), np.array([np.inf, 1.0], F32), np.array([2.0 ** 64 * 1.5, 1.0], F32), np.array([1e-40, 0.0], F32)):
            y = C.maxact(x, 4, fn)
            assert y.shape == x.shape and np.isnan(y).all(), (fn, x)
        for M in (2.0 ** -64, 2.0 ** 64, 1.5 * 2.0 ** 63, 1.5 * 2.0 ** -64):        # the ends of the exact range
            x = np.array([M, M / 2, -M], F32)
            for nb in (2, 24):
                y = C.maxact(x, nb, fn)
                P = 2.0 ** C.scale_exponent(F32(M))
                m = 2.0 ** (nb - 1)
                want = [min(np.rint(M / P * m), m - 1) * P / m, min(np.rint(M / 2 / P * m), m - 1) * P / m,
                        0.0 if fn == "quantized_maxrelu" else max(np.rint(float(F32(0.1) * F32(-M)) / P * m), -m) * P / m]
                assert np.array_equal(y, np.array(want, F32)), (fn, M, nb, y, want)


# ---- the maximum of a sharded batch --------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _max_forward(x):
    """CPU stand-in for a quantized_maxrelu layer with the structure of the GPU op: a padded (zero) image gives the LARGEST
    pre-activation (4.5 everywhere, a real image stays below 3.8: scale 8 against 4), the maximum is taken over this
    shard's VALID rows only and all-reduced, the scale is applied to every row."""
    flat = x.reshape(x.shape[0], -1)
    pre = 2.0 * flat + (4.5 - 8.0 * flat.mean(dim=1, keepdim=True))
    M = shard.allreduce_max_relu(pre, valid_rows=shard.active_valid_rows())
    return torch.from_numpy(C.maxact(pre.numpy(), 4, "quantized_leakymaxrelu", M=F32(M)))[:, :10].contiguous()


def _worker(rank, world, port, total, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        x = torch.rand((total, 4, 4, 3), generator=torch.Generator().manual_seed(2))
        y = shard.sharded_forward(_max_forward, x, rank, world)
        lo, hi, _ = shard.shard_bounds(total, rank, world)
        part = (x * 4 - 2)[lo:hi]
        m = shard.allreduce_max_relu(part)
        # the workspace word quantized_ops all-reduces between its two kernels: bits of this shard's max(x, 0)
        ws = torch.zeros(4, dtype=torch.int32)
        ws[0] = int(np.asarray(part.clamp(min=0).amax().item(), dtype=F32).view(np.int32))
        untouched = shard.allreduce_max(ws.clone())             # outside a sharded context: no exchange
        with shard.sharded():
            shard.allreduce_max(ws)
        neg = shard.allreduce_max_relu(-part.abs() - 1)          # no positive value anywhere: 0, the NaN case
        if rank == 0:
            torch.save({"y": y, "m": m, "ws": ws, "local": untouched, "neg": neg}, out)
    finally:
        dist.destroy_process_group()


def test_two_ranks_find_the_unsplit_maximum(tmp_path):
    for total in (16, 13):                      # even split and ragged (padded) split
        x = torch.rand((total, 4, 4, 3), generator=torch.Generator().manual_seed(2))
        want = _max_forward(x)                  # no sharded context: one process, every row valid
        out = str(tmp_path / ("max_%d.pt" % total))
        mp.spawn(_worker, args=(2, _free_port(), total, out), nprocs=2, join=True)
        got = torch.load(out, weights_only=True)
        assert torch.equal(got["y"], want), total
        ref = (x * 4 - 2).clamp(min=0).amax()
        assert float(got["m"]) == float(ref) and float(got["neg"]) == 0.0
        assert got["ws"][:1].view(torch.float32).item() == float(ref) and got["ws"][1:].tolist() == [0, 0, 0]
        assert got["local"][:1].view(torch.float32).item() <= float(ref)
    # the padding really would win: with every row of the padded shard counted the scale doubles
    x = torch.rand((13, 4, 4, 3), generator=torch.Generator().manual_seed(2))
    padded = torch.cat([x, torch.zeros((1, 4, 4, 3))])
    assert not torch.equal(_max_forward(padded)[:13], _max_forward(x))


# ---- the Python surface --------------------------------------------------------------------------------------------------
def test_abi_constants_and_the_extension_header():
    hdr = open(os.path.join(ROOT, "include", "qnn_abi_maxact.h")).read()
    assert re.search(r"#define QNN_FN_QUANTIZED_MAXRELU\s+8\b", hdr) and re.search(r"#define QNN_FN_QUANTIZED_LEAKYMAXRELU\s+9\b", hdr)
    assert (_abi.FN_QUANTIZED_MAXRELU, _abi.FN_QUANTIZED_LEAKYMAXRELU) == (8, 9) == _abi.MAXACT_FNS
    assert not set(_abi.MAXACT_FNS) & set(_abi.QUANT_FNS)            # not among the activations that carry act_bits
    for word in ("16 ulp", "2^-64", "NaN", "QNN_EUNSUPPORTED"):      # the deviation band, the range and the refusals are stated
        assert word in hdr, word
    ext = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(qnn_[a-z0-9_]+)\s*\(", ext))) == sorted(_abi.EXPORTS_MAXACT)
    assert sorted(_abi.EXPORTS_MAXACT) == ["qnn_maxact_apply_f32", "qnn_maxact_max_f32", "qnn_quantized_maxact_f32"]
    assert not set(_abi.EXPORTS_MAXACT) & set(_abi.EXPORTS + _abi.EXPORTS_QACT + _abi.EXPORTS_DILATION) and len(_abi.EXPORTS) == 29
    lib = _abi.load()
    assert lib.qnn_version() == 4
    # argument checks come before any device call
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    for fn in _abi.MAXACT_FNS:
        assert lib.qnn_quantized_maxact_f32(buf, buf, 0, fn, 4, buf, None) == 0           # n == 0: nothing to launch
        assert lib.qnn_maxact_apply_f32(buf, buf, 0, fn, 4, buf, None) == 0
        for nb in (1, 25):
            assert lib.qnn_quantized_maxact_f32(buf, buf, 4, fn, nb, buf, None) == -1
            assert lib.qnn_maxact_apply_f32(buf, buf, 4, fn, nb, buf, None) == -1
        assert lib.qnn_quantized_maxact_f32(None, buf, 4, fn, 4, buf, None) == -1
        assert lib.qnn_quantized_maxact_f32(buf, buf, 4, fn, 4, None, None) == -1
        # every entry that takes a QNN_FN_* code refuses the two with a reason that names the elementwise entry
        assert lib.qnn_pack_f32(buf, buf, 1, 8, fn, 4, _abi.STORE_I4, None) == _abi.QNN_EUNSUPPORTED
        assert b"qnn_quantized_maxact_f32" in lib.qnn_last_error()
        assert lib.qnn_quantized_act_f32(buf, buf, 4, fn, 4, None) == _abi.QNN_EUNSUPPORTED
        assert b"qnn_quantized_maxact_f32" in lib.qnn_last_error()
    for fn in (_abi.FN_QUANTIZED_TANH, _abi.FN_QUANTIZED_LEAKYRELU, _abi.FN_NONE):
        assert lib.qnn_quantized_maxact_f32(buf, buf, 4, fn, 4, buf, None) == -1
    assert lib.qnn_maxact_max_f32(buf, 4, None, None) == -1


def test_python_surface():
    assert qnn_amd.quantized_maxrelu is quantized_ops.quantized_maxrelu
    assert qnn_amd.quantized_leakymaxrelu is quantized_ops.quantized_leakymaxrelu
    x = torch.zeros(4, 4)
    for bad in (0.3, 0.0, 0.1000001, 1):
        with pytest.raises(ValueError, match="quantized_leakymaxrelu"):
            quantized_ops.quantized_leakymaxrelu(x, 4, alpha=bad)
    for fn in (quantized_ops.quantized_maxrelu, quantized_ops.quantized_leakymaxrelu):
        with pytest.raises(_abi.QnnError):          # a float32 DEVICE tensor is required: there is no CPU path
            fn(x, 4)
        with pytest.raises(TypeError):
            fn(np.zeros((4, 4), F32), 4)
        for word in ("16 ulp", "NaN", "batch"):
            assert word in fn.__doc__ or "see quantized_maxrelu" in fn.__doc__
    # not a fixed-grid clip: the engines materialise it as float32
    for name in C.FNS:
        assert engine._act_code({"op": "act", "fn": name, "nb": 4}) is None
        assert engine.LayerModel._grid({"op": "act", "fn": name, "nb": 4}) is None
    with pytest.raises(ValueError):
        engine._act_code({"op": "act", "fn": "quantized_leakymaxrelu", "nb": 4, "alpha": 0.3})


@pytest.mark.parametrize("fn", C.FNS)
def test_spec_builders_take_the_activation_and_the_packed_engines_refuse_it(fn):
    assert fn in nets.QUANTIZED_ACTIVATIONS and fn in nets.BATCH_SCALED_ACTIVATIONS
    for nt in ("full-qnn", "qbnn", "qtnn"):
        for arch in ("VGG", "RESNET"):
            cf = nets.Config(network_type=nt, wbits=4, abits=3, architecture=arch, nres=1)
            spec = nets.build_spec(cf, 3, quantized_activation=fn, batch_scaled=True)
            with pytest.raises(ValueError, match="batch_scaled=True"):       # the batch dependence is opted into, never implied
                nets.build_spec(cf, 3, quantized_activation=fn)
            acts = [op for op in spec if op["op"] == "act"]
            assert acts and all(a["fn"] == fn and a["nb"] == 3 for a in acts), (nt, arch)
            base = nets.build_spec(cf, 3)
            assert [op["op"] for op in base] == [op["op"] for op in spec]
            assert all(a["fn"] == "quantized_tanh" for a in base if a["op"] == "act")
            for cls in (engine.FusedModel, engine.ResidualFusedModel):
                with pytest.raises(_abi.NotFusable, match="maximum of the whole batch"):
                    cls(spec, device="cpu")
    for nt in ("qnn", "full-bnn", "float"):          # no quantised activation to replace
        spec = nets.build_spec(nets.Config(network_type=nt), 3, quantized_activation=fn, batch_scaled=True)
        assert all(a["fn"] != fn for a in spec if a["op"] == "act")
    for bad in ("quantized_maxtanh", "maxrelu", "", None):
        for flag in (False, True):
            with pytest.raises(ValueError):
                nets.build_spec(nets.Config(), 3, quantized_activation=bad, batch_scaled=flag)
    for per_value in ("quantized_tanh", "quantized_relu", "quantized_leakyrelu"):
        with pytest.raises(ValueError, match="batch_scaled"):
            nets.build_spec(nets.Config(), 3, quantized_activation=per_value, batch_scaled=True)
    assert nets._act_second_moment({"op": "act", "fn": fn, "nb": 4}) > 0


@pytest.mark.parametrize("fn", C.FNS)
def test_a_checkpoints_activation_of_that_name_is_the_op(fn, tmp_path):
    """Activation('quantized_maxrelu' / 'quantized_leakymaxrelu') in a checkpoint: no lambda of the reference shadows these
    names (model_factory.py:19-20 shadows quantized_relu only), so they map to the ops, with nb = abits."""
    import json
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "resnet3_full_44.npz")))
    cfg = json.loads(bytes(d["model_config_json"]).decode())
    acts = [l for l in cfg["config"]["layers"] if l["class_name"] == "Activation" and l["config"]["activation"] == "quantized_relu"]
    assert len(acts) >= 10
    for l in acts[1:]:
        l["config"]["activation"] = fn
    d["model_config_json"] = np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8)
    path = str(tmp_path / "net.npz")
    np.savez(path, **d)
    spec = nets.spec_from_keras_npz(path, 4, 3)
    got = [op for op in spec if op["op"] == "act"]
    assert got[0]["fn"] == "quantized_tanh" and got[0]["nb"] == 3                  # the shadowing lambda stays what it was
    assert len(got) == len(acts) and all(a["fn"] == fn and a["nb"] == 3 for a in got[1:])
    base = nets.spec_from_keras_npz(os.path.join(ROOT, "tests", "golden", "resnet3_full_44.npz"), 4, 3)
    assert [op["op"] for op in base] == [op["op"] for op in spec]
    for cls in (engine.FusedModel, engine.ResidualFusedModel):
        with pytest.raises(_abi.NotFusable, match="maximum of the whole batch"):
            cls(spec, device="cpu")
    d["model_config_json"] = np.frombuffer(json.dumps(cfg).replace(fn, "quantized_maxtanh").encode(), dtype=np.uint8)
    np.savez(path, **d)
    with pytest.raises(ValueError, match="unsupported activation"):
        nets.spec_from_keras_npz(path, 4, 3)
