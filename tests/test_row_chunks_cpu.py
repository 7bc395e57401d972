"""CPU checks of ``_marshal.row_chunks``, the one row-chunk loop of the chunked entry points: the chunks tile the rows in order,
``at`` gives the data pointer of a chunk's rows of any tensor and passes None through."""
import pytest
import torch

from vae_assoc_amd._marshal import row_chunks


@pytest.mark.parametrize("N", [0, 1, 5])
@pytest.mark.parametrize("chunk", [0, 1, 2, 5, 7])
def test_chunks_tile_the_rows_in_order_and_point_at_their_rows(N, chunk):
    tensors = [torch.arange(N, dtype=torch.int32), torch.zeros((N, 3, 2), dtype=torch.float32),
               torch.zeros((N, 4), dtype=torch.float64)]
    nxt = 0
    for r0, n, at in row_chunks(N, chunk):
        assert r0 == nxt and 1 <= n <= max(1, chunk)
        assert n == max(1, chunk) or r0 + n == N               # only the last chunk is short
        for t in tensors:
            assert at(t) == t[r0:r0 + n].data_ptr() == t.data_ptr() + r0 * t.stride(0) * t.element_size()
        assert at(None) is None
        nxt = r0 + n
    assert nxt == N


def test_no_rows_yield_nothing_and_every_chunk_keeps_its_own_rows():
    assert list(row_chunks(0, 4)) == []
    t = torch.arange(5, dtype=torch.int32)
    chunks = list(row_chunks(5, 2))                            # (kept past the loop: ``at`` must not follow the loop variable)
    assert [(r0, n) for r0, n, _ in chunks] == [(0, 2), (2, 2), (4, 1)]
    assert [at(t) for _, _, at in chunks] == [t.data_ptr(), t.data_ptr() + 8, t.data_ptr() + 16]
