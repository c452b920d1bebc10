"""step.pack_eligible: when the frozen teachers of a step run as one pack forward.  Host arithmetic only."""
import itertools

import pytest

from mm_distillnet_amd.step import pack_eligible


@pytest.mark.parametrize("S, B, G, node_whole, packs", [
    (512, 8, 3, True, True), (512, 8, 3, False, True),        # 128 rows per net on the smallest level
    (256, 2, 3, True, False), (256, 2, 3, False, False),      # 8 rows
    (256, 8, 3, True, True), (256, 8, 3, False, False),       # 32 rows: whole 32-row tiles, so the whole-node kernel decides
    (768, 8, 3, True, True), (768, 8, 3, False, False),       # 288 rows, the D4 case
    (320, 8, 3, True, False), (320, 8, 3, False, False),      # S is not a multiple of 128
])
def test_named_geometries(S, B, G, node_whole, packs):
    assert pack_eligible(S, B, G, aug=False, node_whole=node_whole, pack=True) is packs


def test_single_teacher_augmented_step_and_engine_without_pack_never_pack():
    assert pack_eligible(512, 8, 3, aug=False, node_whole=True, pack=True) is True
    assert pack_eligible(512, 8, 1, aug=False, node_whole=True, pack=True) is False
    assert pack_eligible(512, 8, 3, aug=True, node_whole=True, pack=True) is False
    assert pack_eligible(512, 8, 3, aug=False, node_whole=True, pack=False) is False


def test_grid_against_the_expression_step_body_held():
    n = 0
    for S, B, G, aug, node_whole, pack in itertools.product(range(128, 1025, 64), range(1, 17), range(1, 4), (False, True), (False, True),
                                                            (False, True)):
        rows_small = B * (S // 128) ** 2
        use_pack = bool(pack and G > 1 and not aug and S % 128 == 0 and
                        (rows_small % 128 == 0 or (rows_small % 32 == 0 and node_whole)))
        assert pack_eligible(S, B, G, aug, node_whole, pack) is use_pack, (S, B, G, aug, node_whole, pack)
        n += 1
    assert n == 15 * 16 * 3 * 8
