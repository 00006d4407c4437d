"""The guard-band arena (tests/guard_util.py) on device='cpu': the checker can
fail, and names the buffer and the side it failed at."""
import pytest

torch = pytest.importorskip('torch')

from guard_util import ALIGN, FILL_BYTE, GUARD, GUARD_BYTE, Arena, untouched  # noqa: E402

SIZES = (('a', 0), ('b', 1), ('c', 3), ('d', 255), ('e', 4112), ('f', 189 * 3))


def _arena():
    ar = Arena([n for _, n in SIZES], device='cpu')
    return ar, {name: ar.take(name, n) for name, n in SIZES}


def test_sizes_carve_correctly():
    ar, t = _arena()
    prev_end = 0
    for (name, n), (a, b) in zip(SIZES, ar.spans):
        assert t[name].numel() == n == b - a
        assert (ar.base + a) % ALIGN == 0
        assert a - prev_end >= GUARD                    # the front guard (behind the previous rear guard)
        assert bool((ar.raw[a - GUARD:a] == GUARD_BYTE).all())
        assert bool((ar.raw[b:b + GUARD] == GUARD_BYTE).all())   # the rear guard begins at the first byte past the end
        assert bool((t[name] == FILL_BYTE).all())
        if n:
            assert t[name].data_ptr() == ar.base + a == ar.ptr(name).value
        prev_end = b + GUARD
    assert prev_end <= ar.raw.numel()
    assert int(ar.guard_mask().sum()) == ar.raw.numel() - sum(n for _, n in SIZES)
    ar.check('fresh')


def test_typed_and_zeroed_payloads():
    ar = Arena([40, 24, 6], device='cpu')
    f = ar.take('f', 40, torch.float32, (2, 5), fill='zero')
    d = ar.take('d', 24, torch.float64)
    h = ar.take('h', 6, torch.int16, (3,))
    assert f.shape == (2, 5) and bool((f == 0).all()) and d.shape == (3,) and h.dtype == torch.int16
    assert bool(untouched(d).all()) and not bool(untouched(f).any())
    with pytest.raises(AssertionError):
        ar.take('odd', 7, torch.float32)
    with pytest.raises(AssertionError, match='too small'):
        ar.take('big', 1 << 20)


def test_a_payload_written_to_its_last_byte_passes():
    ar, t = _arena()
    for name, _ in SIZES:
        t[name].fill_(0x11)
    ar.check('full payloads')
    assert not bool(untouched(t['d']).any())


@pytest.mark.parametrize('name', ['a', 'b', 'd', 'f'])
def test_one_byte_past_a_payload(name):
    ar, _ = _arena()
    a, b = ar.spans[ar.names.index(name)]
    ar.raw[b] = 0
    with pytest.raises(AssertionError) as e:
        ar.check('past')
    msg = str(e.value)
    assert f"buffer '{name}'" in msg and 'AFTER' in msg and 'offset 0 past its end' in msg and '1 bytes changed' in msg
    assert msg.count("buffer '") == 1 and 'BEFORE' not in msg


@pytest.mark.parametrize('name', ['a', 'b', 'd', 'f'])
def test_one_byte_before_a_payload(name):
    ar, _ = _arena()
    a, b = ar.spans[ar.names.index(name)]
    ar.raw[a - 1] = 0
    with pytest.raises(AssertionError) as e:
        ar.check('before')
    msg = str(e.value)
    assert f"buffer '{name}'" in msg and 'BEFORE' in msg and 'from 1 to 1 bytes before' in msg
    assert msg.count("buffer '") == 1 and 'AFTER' not in msg


@pytest.mark.parametrize('name', ['a', 'c', 'f'])
def test_the_far_ends_of_the_guards(name):
    ar, _ = _arena()
    a, b = ar.spans[ar.names.index(name)]
    ar.raw[b + GUARD - 1] = 1
    with pytest.raises(AssertionError) as e:
        ar.check('far rear')
    msg = str(e.value)
    assert f"buffer '{name}'" in msg and f'offset {GUARD - 1} past its end' in msg and msg.count("buffer '") == 1
    ar.raw[b + GUARD - 1] = GUARD_BYTE
    ar.raw[a - GUARD] = 1
    with pytest.raises(AssertionError) as e:
        ar.check('far front')
    msg = str(e.value)
    assert f"buffer '{name}'" in msg and 'BEFORE' in msg and f'from {GUARD} to {GUARD}' in msg
    assert msg.count("buffer '") == 1
    ar.raw[a - GUARD] = GUARD_BYTE
    ar.check('restored')


def test_count_and_first_offset_of_a_run():
    ar, _ = _arena()
    a, b = ar.spans[ar.names.index('d')]
    ar.raw[b + 5:b + 21] = 7            # one 16-byte store that begins 5 bytes past the end
    with pytest.raises(AssertionError) as e:
        ar.check('run')
    msg = str(e.value)
    assert "buffer 'd' (255 bytes): 16 bytes changed AFTER it, the first at offset 5 past its end, the last at 20" in msg
    assert '0x07' in msg
