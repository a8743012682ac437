"""The host bounds check of a coalesced step's batched KV store (tts_hip_coalesce_store_ok, called by co_prepare
for every member and destination before the destination tables are uploaded): a destination view must lie
inside its member's cache tensor on 4-byte boundaries, or the group is refused and nothing is launched.
Pure arithmetic, checked here without a device and without launching anything."""
import ttship

H, HD, NKV, REPEAT, CTX = 256, 64, 2, 2, 48  # the tiny Orpheus cache: [H * CTX] floats per layer
CACHE = 4 * H * CTX
NE = (HD, NKV, 1, 1)                         # one token's K rows for one repeat copy
NB = (4, 4 * HD * REPEAT, 4 * H, 4 * H)


def off(position, copy):
    return 4 * H * position + 4 * HD * copy


def test_every_real_destination_is_inside():
    for position in (0, 1, CTX - 1):
        for copy in range(REPEAT):
            assert ttship.coalesce_store_ok(off(position, copy), NE, NB, CACHE)


def test_last_destination_ends_exactly_at_the_cache_end():
    end = off(CTX - 1, REPEAT - 1) + 4 + sum((NE[d] - 1) * NB[d] for d in range(4))
    assert end == CACHE
    assert ttship.coalesce_store_ok(off(CTX - 1, REPEAT - 1), NE, NB, end)
    assert not ttship.coalesce_store_ok(off(CTX - 1, REPEAT - 1), NE, NB, end - 4)


def test_one_float_past_the_cache_is_refused():
    assert not ttship.coalesce_store_ok(off(CTX - 1, REPEAT - 1) + 4, NE, NB, CACHE)
    assert not ttship.coalesce_store_ok(off(CTX, 0), NE, NB, CACHE)  # the row after the last position


def test_negative_and_misaligned_offsets_are_refused():
    assert not ttship.coalesce_store_ok(-4, NE, NB, CACHE)
    assert not ttship.coalesce_store_ok(off(3, 1) + 2, NE, NB, CACHE)
    assert not ttship.coalesce_store_ok(off(3, 1), NE, (4, 4 * HD * REPEAT + 2, 4 * H, 4 * H), CACHE)


def test_huge_shapes_do_not_overflow():
    assert not ttship.coalesce_store_ok(0, (HD, 1 << 40, 1 << 20, 1), (4, 1 << 40, 1 << 50, 4), CACHE)
    assert not ttship.coalesce_store_ok((1 << 62), NE, NB, CACHE)
