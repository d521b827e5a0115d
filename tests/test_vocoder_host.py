"""CPU-side checks of the vocoder operator entry points: maa_op_conv_transpose1d and maa_vocoder_create refuse the transposed
convolutions the polyphase GEMMs do not cover, and maa_op_mrf_pair its malformed arguments -- all before the device is touched
(no GPU, no kernel launch)."""
import ctypes

import pytest

from tests import vocoder_ref as R


@pytest.fixture(scope="module")
def lib():
    from audiogpt_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _fake(n=1):
    return ctypes.c_void_p(16 * n)          # a non-null pointer that the argument checks never dereference


def _host():
    buf = (ctypes.c_float * 4)()
    return buf, ctypes.cast(buf, ctypes.POINTER(ctypes.c_float))


def test_conv_transpose1d_entry_names_the_rule_it_refuses_by(lib):
    keep, h = _host()
    assert lib.maa_op_conv_transpose1d(None, None, 3, 32, 5, h, h, 16, 4, 2, 0.1, _fake()) < 0
    assert b"bad op_conv_transpose1d" in lib.maa_last_error()
    for k, s, rule in R.CONVTR_REFUSED:
        assert lib.maa_op_conv_transpose1d(None, _fake(), 3, 32, 5, h, h, 16, k, s, 0.1, _fake()) < 0
        err = lib.maa_last_error()
        assert rule.encode() in err and ("kernel %d, stride %d" % (k, s)).encode() in err, err
    assert lib.maa_op_conv_transpose1d(None, _fake(), 3, 32, 5, h, h, 16, 4, 0, 0.1, _fake()) < 0
    assert b"stride >= 1" in lib.maa_last_error()
    # every shape of the operator tests, and the shipped k = 2 s (even strides), reach the context, which is null here
    for k, s in [(k, s) for _, _, k, s, _ in R.CONVTR] + [(16, 8), (4, 2), (8, 4), (12, 6)]:
        assert lib.maa_op_conv_transpose1d(None, _fake(), 3, 32, 5, h, h, 16, k, s, 0.1, _fake()) < 0
        assert b"null context" in lib.maa_last_error(), (k, s, lib.maa_last_error())


def test_vocoder_create_refuses_an_unsupported_upsampler(lib):
    from audiogpt_amd import _lib
    cfg = _lib.maa_vocoder_config()
    cfg.num_mels, cfg.upsample_initial_channel, cfg.n_upsamples, cfg.n_kernels, cfg.n_dilations = 80, 64, 2, 1, 1
    cfg.resblock_kernel_sizes[0] = 3
    cfg.resblock_dilation_sizes[0][0] = 1
    out = ctypes.c_void_p()
    for k, s, rule in R.CONVTR_REFUSED:
        cfg.upsample_rates[0], cfg.upsample_kernel_sizes[0] = 8, 16
        cfg.upsample_rates[1], cfg.upsample_kernel_sizes[1] = s, k
        assert lib.maa_vocoder_create(None, ctypes.byref(cfg), None, 0, ctypes.byref(out)) < 0
        assert rule.encode() in lib.maa_last_error(), lib.maa_last_error()
    cfg.upsample_rates[1], cfg.upsample_kernel_sizes[1] = 2, 4
    assert lib.maa_vocoder_create(None, ctypes.byref(cfg), None, 0, ctypes.byref(out)) < 0
    assert b"null context" in lib.maa_last_error()


def test_mrf_pair_entry_rejects_bad_arguments(lib):
    keep, h = _host()
    assert lib.maa_op_mrf_pair(None, None, 3, 32, 5, h, h, 3, 1, 0.1, h, h, 3, 1, 0.1, 1.0, 0, _fake()) < 0
    assert b"bad op_mrf_pair" in lib.maa_last_error()
    assert lib.maa_op_mrf_pair(None, _fake(), 3, 32, 0, h, h, 3, 1, 0.1, h, h, 3, 1, 0.1, 1.0, 0, _fake()) < 0
    assert b"bad op_mrf_pair" in lib.maa_last_error()
    assert lib.maa_op_mrf_pair(None, _fake(), 3, 32, 5, h, h, 4, 1, 0.1, h, h, 3, 1, 0.1, 1.0, 0, _fake()) < 0
    assert b"k1 must be odd" in lib.maa_last_error()
    assert lib.maa_op_mrf_pair(None, _fake(), 3, 32, 5, h, h, 3, 1, 0.1, h, h, 3, 0, 0.1, 1.0, 0, _fake()) < 0
    assert b"k2 must be odd" in lib.maa_last_error()
    # a ResBlock2 step ignores k2 / d2; well-formed arguments reach the context, which is null here
    assert lib.maa_op_mrf_pair(None, _fake(), 3, 32, 5, h, None, 3, 1, 0.1, None, None, 0, 0, 0.0, 1.0, 1, _fake()) < 0
    assert b"null context" in lib.maa_last_error()
    assert lib.maa_op_mrf_pair(None, _fake(), 3, 32, 5, h, h, 11, 5, 0.1, h, h, 11, 1, 0.1, 1.0 / 3.0, 1, _fake()) < 0
    assert b"null context" in lib.maa_last_error()
