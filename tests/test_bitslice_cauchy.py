"""The bit-sliced encode networks of the Cauchy matrix (0xfec_amd/gen_bitslice.py CAUCHY_SHAPES,
emitted into csrc/fec_bitslice.inc with the kind tag 1), checked on the CPU against the definition
model (tests/cauchy_model.py), as tests/test_bitslice.py checks the default matrix's against the oracle:

  - the generator's Cauchy rows equal the model's matrix;
  - the whole kernel algorithm restated in numpy (two 16-byte chunks per lane as 8 dwords, the
    delta-swap stages of bit_transpose8, the network, the transpose back) gives the model's parity;
  - the networks' op counts stay within the kernel's VALU budget;
  - the committed .inc carries both kinds' instantiations.
Parity of the GPU kernel itself is tests/test_gpu_cauchy.py."""
import os

import numpy as np
import pytest

import cauchy_model as cm
from test_bitslice import ROOT, bit_transpose8, gen


@pytest.mark.parametrize("k,m,g", gen.CAUCHY_SHAPES)
def test_generator_rows_are_the_models(k, m, g):
    assert gen.cauchy_parity_rows(k, m) == [list(map(int, r)) for r in cm.matrix(k, m)[k:]]


def test_cauchy_shapes_are_the_bit_sliced_ones():
    assert [(k, m) for k, m, _ in gen.CAUCHY_SHAPES] == [(16, 8), (20, 10)]


@pytest.mark.parametrize("k,m,g", gen.CAUCHY_SHAPES)
def test_bitsliced_cauchy_encode_equals_model(k, m, g):
    rng = np.random.default_rng(k * 100 + m + 1)
    B = 96
    data = rng.integers(0, 256, (B, k, 32), dtype=np.uint8)
    data[0] = 0xFF            # all-ones and single-bit columns
    data[1, :, :8] = 1 << np.arange(8, dtype=np.uint8)
    data[1, :, 8:] = 0
    want = cm.encode(cm.matrix(k, m), data)
    # a lane's 8 dwords per shard: chunk c (dwords 0-3) and chunk c + h (dwords 4-7)
    words = data.copy().view("<u4")            # (B, k, 8)
    planes = []
    for j in range(k):
        planes += bit_transpose8([words[:, j, d] for d in range(8)])
    ops = gen.schedule(k, m, g, rows=gen.cauchy_parity_rows(k, m))
    y = gen.run_schedule(ops, planes, 8 * m)
    got = np.zeros((B, m, 8), dtype=np.uint32)
    for r in range(m):
        out = bit_transpose8(y[8 * r:8 * r + 8])
        for d in range(8):
            got[:, r, d] = out[d]
    assert np.array_equal(got.view(np.uint8).reshape(B, m, 32), want)
    # and it is not the default matrix's network
    assert ops != gen.schedule(k, m, g)


def test_cauchy_network_op_counts():
    # what the kernel's VALU budget assumes (three-input XOR folds)
    rows = gen.cauchy_parity_rows
    assert gen.op_count(gen.schedule(16, 8, 4, rows=rows(16, 8))) <= 1210
    assert gen.op_count(gen.schedule(20, 10, 4, rows=rows(20, 10))) <= 1900


def test_default_schedule_is_unchanged_by_the_rows_argument():
    for k, m, g in gen.SHAPES:
        assert gen.schedule(k, m, g) == gen.schedule(k, m, g, rows=gen.parity_rows(k, m))


def test_include_holds_both_kinds():
    text = open(os.path.join(ROOT, "0xfec_amd", "csrc", "fec_bitslice.inc")).read()
    for k, m, g in gen.SHAPES:
        assert "struct BsShape<%d, %d> {" % (k, m) in text
        assert "bs_grp<%d, %d, 0>(" % (k, m) in text
    for k, m, g in gen.CAUCHY_SHAPES:
        assert "struct BsShape<%d, %d, 1> {" % (k, m) in text
        for gi in range(k // g):
            assert "bs_grp<%d, %d, %d, 1>(" % (k, m, gi) in text
