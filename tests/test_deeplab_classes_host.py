"""The class tables a DeepLabV3 model stores through its u8 final op (models.class_lut3 /
class_lut_binary): pure NumPy, no GPU. The reference's convention (models.py:56-58: argmax ids 0, 1 ->
1 road, ids 2, 9 -> 0 flat non-road, the rest -> 2; models.py:79-80: ids 0, 1 -> 1, the rest -> 0) is
restated here as literal tables of its 15 classes."""
import numpy as np
import pytest

from bugcar_image_segmentation_amd.models import class_lut3, class_lut_binary

REF_LUT3 = [1, 1, 0, 2, 2, 2, 2, 2, 2, 0, 2, 2, 2, 2, 2]
REF_BINARY = [1, 1] + [0] * 13


def test_reference_tables():
    lut = class_lut3(15, (0, 1), (2, 9))
    assert lut.dtype == np.uint8 and lut.tolist() == REF_LUT3
    ids = np.arange(15)
    # models.py:56-58 as it is written: ones * 2, then the two where()s
    where = np.where((ids == 0) | (ids == 1), 1, np.where((ids == 2) | (ids == 9), 0, 2))
    assert np.array_equal(lut, where)
    b = class_lut_binary(15, (0, 1))
    assert b.dtype == np.uint8 and b.tolist() == REF_BINARY
    assert np.array_equal(b, ((ids == 0) | (ids == 1)).astype(np.uint8))     # models.py:79-80


def test_other_label_sets():
    assert class_lut3(1, (), ()).tolist() == [2]
    assert class_lut3(4, [3], []).tolist() == [2, 2, 2, 1]
    assert class_lut3(256, range(0, 256, 2), [1]).tolist() == [1, 0] + [1, 2] * 127
    assert class_lut_binary(3, np.array([2])).tolist() == [0, 0, 1]
    assert class_lut_binary(256, ()).tolist() == [0] * 256


@pytest.mark.parametrize("args", [
    (15, (0, 1), (1, 9)),        # an id both road and flat
    (15, (0, 0), (2,)),          # a repeated id
    (15, (15,), ()),             # out of range
    (15, (), (-1,)),
    (15, (0.5,), ()),            # not an integer
    (0, (), ()),                 # class counts a byte cannot index
    (257, (0,), ()),
])
def test_lut3_refusals(args):
    with pytest.raises(ValueError):
        class_lut3(*args)


@pytest.mark.parametrize("args", [(15, (15,)), (15, (-1,)), (15, (1, 1)), (0, ()), (257, (0,))])
def test_binary_refusals(args):
    with pytest.raises(ValueError):
        class_lut_binary(*args)
