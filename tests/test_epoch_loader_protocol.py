"""The epoch protocol that the four loaders of `sampling` share, on CPU tensors with the device's draws replaced by stubs: which rows
an epoch serves and in which order, that the columns and the negatives travel with their rows, the batch sizes without `shuffle` and
`drop_last`, and the epoch counter.  What the draws put into the negatives is the business of the GPU tests of each sampler."""
import pytest
import torch

N, BATCH, SEED, COLUMNS = 103, 10, 5, 7
ROWS = torch.arange(N)
COLS = tuple(ROWS * 10 + q for q in range(COLUMNS))                 # year, u_id, age, sex, month, day, dow
ITEMS = ROWS + 1000


def _negatives(epoch: int, width: int) -> torch.Tensor:
    """The stubs' draw of an epoch, [N, width]: a value says which row, which slot and which epoch it belongs to."""
    return 100000 * (epoch + 1) + ROWS[:, None] * 10 + torch.arange(width)


def _loader(name, m, monkeypatch, **options):
    """(loader, width of a row's negatives, whether they are redrawn per epoch).  `HardTripletLoader` draws through
    `sampling._hard_draw`; the loaders with m negatives per row are set up by the private base alone, without the seen sets and
    the prepared weights that need the device, and fill their negatives through a stubbed `_draw`."""
    from seoul_tourism_recommendation_ngcf_amd import sampling
    cls = getattr(sampling, name)
    if name == "TripletLoader":
        return cls(ROWS, ITEMS, _negatives(0, 1)[:, 0], COLS, batch_size=BATCH, **options), 1, False
    if name == "HardTripletLoader":
        calls = []

        def draw(users, user_emb, item_emb, seen, m_, seed_e, chunk=None, out=None):
            calls.append(seed_e)
            assert m_ == m and seed_e == sampling.fmix(9 + len(calls) - 1)
            return out.copy_(_negatives(len(calls) - 1, 1)[:, 0])
        monkeypatch.setattr(sampling, "_hard_draw", draw)
        tables = lambda: (torch.zeros(N, 4), torch.zeros(1000 + N, 4))  # noqa: E731
        return cls(ROWS, ITEMS, COLS, batch_size=BATCH, tables=tables, m=m, seed=9, **options), 1, True
    loader = cls.__new__(cls)
    sampling._EpochLoader.__init__(loader, name, ROWS, COLS, (ITEMS,), batch_size=BATCH, m=m, m_max=64,
                                   **{**dict(shuffle=True, drop_last=True, generator=None), **options})
    loader.neg = torch.empty((N, m), dtype=torch.int64)
    monkeypatch.setattr(cls, "_draw", lambda self: self.neg.copy_(_negatives(self.epoch, m)))
    return loader, m, True


def _check_batches(batches, rows, negatives):
    """Every batch is (*columns[b], items[b], neg[b].reshape(-1)) of int64 for the rows `rows`, in their order."""
    assert all(len(b) == COLUMNS + 2 and all(c.dtype == torch.int64 and c.dim() == 1 for c in b) for b in batches)
    for q in range(COLUMNS):
        assert torch.equal(torch.cat([b[q] for b in batches]), COLS[q][rows])
    assert torch.equal(torch.cat([b[COLUMNS] for b in batches]), ITEMS[rows])
    width = negatives.shape[1]
    assert all(b[-1].shape == (b[0].numel() * width,) for b in batches)                  # the negatives of a row lie next to each other
    assert torch.equal(torch.cat([b[-1] for b in batches]).view(-1, width), negatives[rows])


CASES = [("TripletLoader", 1), ("HardTripletLoader", 1), ("HardTripletLoader", 4), ("NegativesLoader", 1), ("NegativesLoader", 4),
         ("WeightedNegativesLoader", 1), ("WeightedNegativesLoader", 4)]


@pytest.mark.parametrize("name,m", CASES)
def test_a_shuffled_epoch_serves_the_generators_permutation(name, m, monkeypatch):
    loader, width, redrawn = _loader(name, m, monkeypatch, generator=torch.Generator().manual_seed(SEED))
    assert len(loader) == N // BATCH
    again = torch.Generator().manual_seed(SEED)                      # one randperm per epoch from the same stream: epoch 2 continues it
    for epoch in range(2):
        batches = list(loader)
        assert [int(b[0].numel()) for b in batches] == [BATCH] * (N // BATCH)
        rows = torch.randperm(N, generator=again)[:N // BATCH * BATCH]
        _check_batches(batches, rows, _negatives(epoch if redrawn else 0, width))
        # the counter of the loaders that redraw; TripletLoader, which redraws nothing, had none before it shared their base
        assert getattr(loader, "epoch", epoch + 1) == epoch + 1


@pytest.mark.parametrize("name,m", CASES)
def test_an_unshuffled_epoch_serves_every_row_in_order(name, m, monkeypatch):
    g = torch.Generator().manual_seed(SEED)
    state = g.get_state()
    loader, width, redrawn = _loader(name, m, monkeypatch, shuffle=False, drop_last=False, generator=g)
    assert len(loader) == N // BATCH + 1
    for epoch in range(2):
        batches = list(loader)
        assert [int(b[0].numel()) for b in batches] == [BATCH] * (N // BATCH) + [N % BATCH]
        _check_batches(batches, ROWS, _negatives(epoch if redrawn else 0, width))
        assert getattr(loader, "epoch", epoch + 1) == epoch + 1
    assert torch.equal(g.get_state(), state)                         # no permutation is drawn
