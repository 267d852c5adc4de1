"""The schedule of a streamed load (musc_stream_plan: the pieces of the upload and the batches of the pass that
consumes it) against its rules, through the device-free entry point -- no GPU.

The bound on neighbouring batches: the rule is "no batch holds more than twice the reads of the batch after it" for
the schedule before its ends are rounded to whole wave-tiles.  Rounding moves an end by less than 64 reads, so the
later batch may have lost up to 64 reads to it: size[i] <= 2 * (size[i + 1] + 64)."""
import numpy as np
import pytest

from muscato_amd.api import stream_plan

BATCHES = [257, 320, 4096, 70001, 16 << 20]
LENS = [31, 90, 100, 150]


def up64(x):
    return (x + 63) // 64 * 64


def read_counts(batch):
    piece = up64(max(batch // 4, 64))
    return sorted({0, 1, 63, 64, 65, piece - 1, piece, piece + 1, batch - 64, batch, batch + 1, 44801234, 500000000})


CASES = [(n, b, L) for b in BATCHES for n in read_counts(b) for L in LENS
         if n // up64(max(b // 4, 64)) <= 10 ** 6]  # (more than 10^6 pieces only repeat the pattern)


@pytest.mark.parametrize("nreads,batch,fixed_len", CASES)
def test_plan_rules(nreads, batch, fixed_len):
    p = stream_plan(nreads, fixed_len, batch)
    ends = [int(e) for e in p["piece_ends"]]
    bends = [int(e) for e in p["batch_ends"]]
    if nreads == 0:
        assert ends == [] and bends == []
        return
    assert all(a < b for a, b in zip(ends, ends[1:])) and ends[0] > 0, "piece ends not strictly increasing"
    assert ends[-1] == nreads and bends[-1] == nreads
    assert all(e % 64 == 0 for e in ends[:-1])
    assert set(bends) <= set(ends), "a batch end that is no piece end"
    sizes = [b - a for a, b in zip([0] + bends, bends)]
    last_max = max(64, up64(batch // 16))
    if nreads > last_max:
        assert sizes[-1] <= last_max, "the last batch holds %d reads" % sizes[-1]
    else:
        assert len(ends) == 1 and len(bends) == 1, "a tiny read set is one piece and one batch"
    for a, b in zip(sizes, sizes[1:]):
        assert a <= 2 * (b + 64), "a batch of %d reads before one of %d" % (a, b)
    assert max(sizes) <= up64(batch)
    assert len(bends) <= p["planned_batches"] <= nreads // batch + 8
    # whole bytes of the 2-bit stream at every piece boundary
    assert all(e * fixed_len % 4 == 0 for e in ends[:-1])


def test_flagship_schedule():
    """cfg3's read count at the default batch size: one full batch, then the taper -- about five batches more than
    the uniform schedule's three, the last one under 2^20 reads."""
    p = stream_plan(44801234, 100)
    sizes = np.diff(np.concatenate([[0], p["batch_ends"].astype(np.int64)]))
    assert sizes[0] == 16 << 20 and 6 <= len(sizes) <= 8 and sizes[-1] <= 1 << 20
    assert p["planned_batches"] == len(sizes)


def test_refused_read_sets():
    with pytest.raises(ValueError):
        stream_plan(2 ** 32 - 16, 100)  # no 32-bit read index for these
    with pytest.raises(ValueError):
        stream_plan(10, 70000)          # longer than a record holds
