"""CPU-only checks of the device validation-metrics entry points (csrc/postprocess.hip): the workspace size queries answer without a GPU
and grow with B * H * W as ocrs_hip.h documents, unsupported shapes are refused, and the device functions have no CPU fallback."""
import pytest
import torch


def test_postprocess_size_queries_work_without_gpu():
    from ocrs_models_amd._lib import lib

    L = lib()
    assert L.cc_quads_capacity(1, 1) == 1 and L.cc_quads_capacity(3, 5) == 2 * 3 and L.cc_quads_capacity(1024, 1024) == 512 * 512
    for q in (L.cc_quads_ws_bytes, L.mask_metrics_ws_bytes):
        assert q(1, 1, 1) > 0 and q(1, 1, 97) > 0 and q(1, 63, 1) > 0
        base = q(1, 256, 256)
        assert q(2, 256, 256) >= 2 * base - 4096          # linear in B (up to alignment)
        assert q(1, 512, 256) >= 2 * base - 4096          # and in H * W
        assert q(4, 512, 512) >= 16 * base - 16 * 4096
        assert q(4, 512, 512) <= 16 * base + 16 * 4096
        assert q(0, 64, 64) == 0 and q(1, 0, 64) == 0 and q(1, 64, 0) == 0
        assert q(1, 65536, 65536) == 0                    # per-image indices would leave 32 bits
    # the end-to-end workspace holds the labelling workspace plus two quad buffers of the capacity
    assert L.mask_metrics_ws_bytes(2, 128, 128) >= L.cc_quads_ws_bytes(2, 128, 128) + 2 * 2 * L.cc_quads_capacity(128, 128) * 32
    assert L.box_match_ws_bytes(3, 100, 64) > 0 and L.box_match_ws_bytes(1, 100, 0) == 0


def test_device_postprocess_has_no_cpu_fallback():
    from ocrs_models_amd import postprocess as pp

    m = torch.zeros(1, 1, 16, 16)
    with pytest.raises(RuntimeError):
        pp.batch_mask_metrics(m, m)
    with pytest.raises(RuntimeError):
        pp.extract_cc_quads_device(m[0])
    with pytest.raises(ValueError):
        pp.batch_mask_metrics(torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 8, 9))
