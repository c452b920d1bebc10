"""CPU: mm_distillnet_amd.pyramid.Pyramid, the row layout of the pyramid row buffers (engine._bifpn, the heads, step._attention)."""
import torch

from mm_distillnet_amd.pyramid import Pyramid


def test_small_padded_pyramid():
    """B = 2 at 32^2 .. 2^2 (a 256^2 input): the 4^2 and 2^2 levels end inside a 128-row tile"""
    p = Pyramid(2, [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)])
    assert p.B == 2 and p.sizes == [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)]
    assert p.rows == [2048, 512, 128, 32, 8]
    assert p.row0 == [0, 2048, 2560, 2688, 2816, 2944]
    assert p.total == 2944 and p.padded is True
    buf = torch.arange(p.total)
    lev = p.levels(buf)
    assert len(lev) == 5
    for l, (lo, n) in enumerate([(0, 2048), (2048, 512), (2560, 128), (2688, 32), (2816, 8)]):
        assert torch.equal(lev[l], torch.arange(lo, lo + n))
        assert torch.equal(p.level(buf, l), lev[l])
    assert lev[0].data_ptr() == buf.data_ptr()            # views of the buffer, not copies
    assert list(p.desc) == [5, 2, 32, 32, 16, 16, 8, 8, 4, 4, 2, 2]
    assert list(p.head_desc(3)) == [3, 2, 32, 32, 16, 16, 8, 8]
    assert p.head_desc(3) is p.head_desc(3)               # built once
    assert p.head_desc(5) is p.desc and list(p.head_desc(5)) == list(p.desc)


def test_unpadded_pyramid():
    """B = 8 at 64^2 .. 4^2 (a 512^2 input): every level is a whole number of tiles"""
    p = Pyramid(8, [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4)])
    assert p.rows == [32768, 8192, 2048, 512, 128]
    assert p.row0 == [0, 32768, 40960, 43008, 43520, 43648]
    assert p.total == 43648 and p.padded is False
    assert [v.shape[0] for v in p.levels(torch.zeros(p.total, 3))] == p.rows
