"""The number key of the results order (musc_results_number_key) and the Python surface of the results
stage.  No GPU: the key is host arithmetic, the Engine methods are only looked up."""
import random

import pytest

from muscato_amd import Engine, api, build as mbuild, number_key


@pytest.fixture(scope="module", autouse=True)
def _built():
    mbuild.build()


def _text(p):
    return b"%d\t%d" % p


EDGES = [(p, n) for p in (0, 1, 8, 9, 10, 11, 98, 99, 100, 101, 999, 1000, 4294967294, 4294967295)
         for n in (0, 1, 9, 10, 11, 99, 100, 65534, 65535)]


def test_number_key_orders_as_the_decimal_text():
    rng = random.Random(7)
    pairs = set(EDGES)
    while len(pairs) < len(EDGES) + 2000:
        # every digit count of pos and nmiss, not just the large values a uniform draw gives
        pairs.add((rng.randrange(10 ** rng.randint(1, 10)) % (1 << 32), rng.randrange(10 ** rng.randint(1, 5)) % 65536))
    pairs = sorted(pairs)
    by_key = sorted(pairs, key=lambda p: number_key(*p))
    by_text = sorted(pairs, key=_text)
    assert by_key == by_text
    assert len({number_key(*p) for p in pairs}) == len(pairs)  # distinct texts, distinct keys


@pytest.mark.parametrize("lo,hi", [(9, 10), (99, 100), (1, 10), (4294967295, 65535)])
def test_number_key_around_a_digit_boundary(lo, hi):
    # "10" < "9" and "1" < "10" (a tab is below '0'), in the pos field and in the nmiss field
    for a, b in [((lo, 0), (hi, 0)), ((5, lo % 65536), (5, hi % 65536)), ((lo, 65535), (hi, 0))]:
        assert (number_key(*a) < number_key(*b)) == (_text(a) < _text(b)), (a, b)
    assert number_key(4294967295, 65535) < 1 << 60
    assert number_key(9, 0) > number_key(10, 65535)
    assert number_key(1, 65535) < number_key(10, 0)


def test_number_key_rejects_six_digits_of_nmiss():
    with pytest.raises(ValueError):
        number_key(0, 100000)


def test_engine_has_the_results_methods():
    for name in ("set_gene_text", "set_read_text", "results_order", "results_hits", "results_text"):
        assert callable(getattr(Engine, name)), name
    assert callable(api.number_key)
