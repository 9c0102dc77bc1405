"""CPU tests of the tensor checks in ``_hip`` that stand between a caller's tensor and a raw pointer handed to a kernel:
``expect``, and ``expect_map_pair`` / ``out_view`` built on it.  Neither the built library nor a GPU is needed."""
import pytest
import torch

from oct_image_segmentation_models_amd._hip import OctError, expect, expect_map_pair, out_view

CPU = torch.device("cpu")
U8 = dict(device=CPU, dtype=torch.uint8)


def test_expect_accepts_what_matches():
    t = torch.zeros((3, 4, 5), dtype=torch.uint8)
    expect(t, "t", shape=(3, 4, 5), **U8)
    expect(t, "t", shape=(None, 4, 5), **U8)                                    # None matches any extent
    expect(t[:2], "t", shape=(None, 4, 5), **U8)                                # a leading slice is still contiguous
    expect(t[:0], "t", shape=(None, 4, 5), **U8)
    expect(t, "t", shape=(None, None, None), **U8)
    expect(t, "t", numel=60, **U8)
    expect(t.view(3, 4, 5, 1), "t", numel=60, **U8)                             # the (B,H,W[,1]) form compares sizes
    expect(t, "t", shape=(3, None, 5), numel=60, **U8)
    expect(t, "t", device=CPU, dtype=(torch.int16, torch.uint8), shape=(3, 4, 5))   # one of several dtypes


@pytest.mark.parametrize("bad,kw", [
    (torch.zeros((3, 4, 5), dtype=torch.int8), dict(shape=(None, 4, 5))),                   # wrong dtype
    (torch.zeros((3, 4, 5), dtype=torch.float32), dict(numel=60)),
    (torch.zeros((3, 4, 10), dtype=torch.uint8)[:, :, ::2], dict(shape=(None, 4, 5))),      # non-contiguous view
    (torch.zeros((3, 5, 4), dtype=torch.uint8).transpose(1, 2), dict(numel=60)),
    (torch.zeros((3, 4), dtype=torch.uint8), dict(shape=(None, 4, 5))),                     # wrong rank
    (torch.zeros((3, 4, 5, 1), dtype=torch.uint8), dict(shape=(None, 4, 5))),
    (torch.zeros((), dtype=torch.uint8), dict(shape=(None,))),
    (torch.zeros((3, 4, 6), dtype=torch.uint8), dict(shape=(None, 4, 5))),                  # a wrong fixed extent
    (torch.zeros((2, 4, 5), dtype=torch.uint8), dict(shape=(3, 4, 5))),
    (torch.zeros((3, 4, 5), dtype=torch.uint8), dict(numel=61)),                            # a mismatched numel
    (torch.zeros((3, 4, 5), dtype=torch.uint8), dict(shape=(None, 4, 5), numel=59)),
], ids=lambda v: None if isinstance(v, torch.Tensor) else "-".join(f"{k}{v[k]}" for k in v))
def test_expect_refuses(bad, kw):
    with pytest.raises(OctError) as e:
        expect(bad, "the argument", **kw, **U8)
    assert "the argument" in str(e.value) and "uint8" in str(e.value) and "cpu" in str(e.value)
    assert str(tuple(bad.shape)) in str(e.value)


def test_expect_refuses_another_device():
    with pytest.raises(OctError):
        expect(torch.zeros((3,), dtype=torch.uint8), "t", device=torch.device("cuda:0"), dtype=torch.uint8, shape=(3,))


def test_expect_map_pair_and_out_view():
    geom = dict(device=CPU, batch=3, H=4, W=5)
    maps = torch.zeros((3, 4, 5), dtype=torch.uint8)
    assert expect_map_pair(maps, maps.clone(), **geom) == 3 and expect_map_pair(maps[:1], maps[1:2], **geom) == 1
    for pred, gt in ((maps, maps[:2]), (maps[:0], maps[:0]), (torch.zeros((4, 4, 5), dtype=torch.uint8),) * 2,
                     (maps, maps.int()), (maps.transpose(1, 2), maps), (maps, torch.zeros((3, 4, 6), dtype=torch.uint8))):
        with pytest.raises(OctError):
            expect_map_pair(pred, gt, **geom)
    own = torch.zeros((3, 7), dtype=torch.int32)
    assert out_view(None, own, 2).data_ptr() == own.data_ptr() and out_view(None, own, 2).shape == (2, 7)
    mine = torch.zeros((2, 7), dtype=torch.int32)
    assert out_view(mine, own, 2) is mine
    for bad in (torch.zeros((3, 7), dtype=torch.int32), torch.zeros((2, 7), dtype=torch.int64),
                torch.zeros((2, 14), dtype=torch.int32)[:, ::2], torch.zeros((2, 8), dtype=torch.int32)):
        with pytest.raises(OctError):
            out_view(bad, own, 2)
