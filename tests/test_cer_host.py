"""CPU-only checks of the device character-error-rate path (csrc/rec_cer.hip): the C ABI is declared and exported, the workspace queries
answer without a GPU, and the Python surface exists and refuses CPU tensors."""
import ctypes
import inspect

import pytest
import torch

NEW_SYMBOLS = ("ocrs_edit_distance", "ocrs_edit_distance_ws_bytes", "ocrs_ctc_cer_update", "ocrs_ctc_cer_ws_bytes")


def test_cer_entry_points_are_declared_and_exported():
    from ocrs_models_amd import build as b
    from ocrs_models_amd._lib import ARG_NAMES, HEADER_PATH, LIB_PATH, lib, parse_header

    b.build(verbose=False)
    sigs = parse_header(HEADER_PATH)
    dll = ctypes.CDLL(LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in sigs, name
        assert hasattr(dll, name), name
    assert sigs["ocrs_ctc_cer_update"] == ("i", "pppppppp" + "iiii" + "s")
    assert sigs["ocrs_edit_distance"] == ("i", "ppi" + "ppi" + "pi" + "pp" + "i" + "s")
    assert ARG_NAMES["ocrs_ctc_cer_ws_bytes"] == ["T", "N", "Lpitch"]
    header = open(HEADER_PATH).read()
    for cite in ("train_rec.py:29-68", "datasets/util.py:132-177"):
        assert cite in header
    L = lib()
    # arg-max, collapsed labels and boundary column [N][T] + compacted targets [N][Lpitch], int32
    assert L.ctc_cer_ws_bytes(101, 256, 128) == 256 * (3 * 101 + 128) * 4
    assert L.ctc_cer_ws_bytes(2048, 4, 2048) == 4 * (3 * 2048 + 2048) * 4  # T is not capped below 2048
    assert L.ctc_cer_ws_bytes(0, 4, 8) == 0 and L.ctc_cer_ws_bytes(4, 0, 8) == 0 and L.ctc_cer_ws_bytes(4, 4, -1) == 0
    assert L.edit_distance_ws_bytes(3, 2047) == 3 * 2047 * 4 and L.edit_distance_ws_bytes(0, 5) == 0
    # argument checks happen before any launch: no GPU needed to see them
    assert L._raw_ocrs_ctc_cer_update(None, None, None, None, None, None, None, None, 4, 4, 4, 4, None) == 1
    assert L._raw_ocrs_edit_distance(None, None, 4, None, None, 4, None, 0, None, None, 1, None) == 1


def test_device_stats_surface_exists_and_refuses_cpu_tensors():
    import ocrs_models_amd as oa
    from ocrs_models_amd import text, train_rec

    stats = text.DeviceRecognitionAccuracyStats()
    for method in ("update", "update_async", "char_error_rate", "stats_dict"):
        assert callable(getattr(stats, method)) and hasattr(text.RecognitionAccuracyStats, method)
    assert stats.char_errors == 0 and stats.total_chars == 0  # nothing queued yet: no device needed
    targets = torch.tensor([[1, 2, 0]], dtype=torch.int32)
    lp = torch.zeros(5, 1, 97).log_softmax(-1)
    with pytest.raises(RuntimeError):
        stats.update(targets, [2], lp, [5])
    with pytest.raises(RuntimeError):
        stats.update_async(targets, [2], lp, [5])
    with pytest.raises(RuntimeError):
        text.edit_distance_device(targets, [2], targets, [2])
    assert oa.text.DEFAULT_ALPHABET and text.alphabet_codes(text.DEFAULT_ALPHABET) is None  # 96 distinct characters: identity
    assert text.alphabet_codes("aab") == [0, 1, 1, 3]
    for fn in (train_rec.train, train_rec.test):
        p = inspect.signature(fn).parameters["stats"]
        assert p.default == "host"
    assert list(inspect.signature(train_rec.train).parameters)[:5] == ["epoch", "device", "dataloader", "model", "optimizer"]
    assert list(inspect.signature(train_rec.test).parameters)[:4] == ["device", "dataloader", "model", "preview"]
    assert isinstance(train_rec.make_stats("host"), text.RecognitionAccuracyStats)
    assert isinstance(train_rec.make_stats("device"), text.DeviceRecognitionAccuracyStats)
    with pytest.raises(ValueError):
        train_rec.make_stats("gpu")
