"""The serving scaffold (`serving.py`) on the CPU: the mode and grad state an entry point leaves behind, the chunking and the id
defaults, against a stub model whose `propagate` records its argument and sets two small tables."""
import pytest
import torch

from seoul_tourism_recommendation_ngcf_amd import serving


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.seen = []

    def propagate(self, year_idx):
        self.seen.append(year_idx)
        self.all_users_emb, self.all_items_emb = torch.arange(15.0).reshape(5, 3), torch.arange(6.0).reshape(2, 3)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("grad", [True, False])
def test_inference_restores_the_callers_mode_and_grad_state(training, grad):
    m = _Stub().train(training)
    with torch.set_grad_enabled(grad):
        with serving.inference(m):
            assert not m.training and not torch.is_grad_enabled()
        assert m.training is training and torch.is_grad_enabled() is grad


@pytest.mark.parametrize("training", [True, False])
def test_inference_restores_the_mode_when_the_body_raises(training):
    m = _Stub().train(training)
    boom = IndexError("a user id lies outside")
    with torch.enable_grad():
        with pytest.raises(IndexError) as caught:
            with serving.inference(m):
                raise boom
        assert caught.value is boom                                     # the body's exception, unchanged
        assert m.training is training and torch.is_grad_enabled()


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 9])                        # 0, 1, size - 1, size, size + 1, 2 size + 1
def test_chunks_cover_the_range_once_and_in_order(n):
    size = 4
    got = list(serving.chunks(n, size))
    assert all(isinstance(sl, slice) and 0 < sl.stop - sl.start <= size for sl in got)
    assert [i for sl in got for i in range(n)[sl]] == list(range(n))
    assert len(got) == -(-n // size)


def test_chunks_take_any_size_int_accepts():
    want = list(serving.chunks(9, 4))
    assert want == [slice(0, 4), slice(4, 8), slice(8, 9)]
    for size in (4.0, torch.tensor(4), "4"):
        assert list(serving.chunks(9, size)) == want


def test_ids_or_all():
    every = serving.ids_or_all(None, 7, torch.device("cpu"))
    assert every.dtype == torch.int64 and torch.equal(every, torch.arange(7))
    given = torch.tensor([[4, 0, 6], [6, 1, 2]], dtype=torch.int32)
    flat = serving.ids_or_all(given, 7, torch.device("cpu"))
    assert flat.dtype == torch.int64 and flat.shape == (6,) and flat.tolist() == [4, 0, 6, 6, 1, 2]


def test_propagated_names_the_models_tables():
    m = _Stub()
    t = serving.propagated(m, 3)
    assert m.seen == [3]
    assert t.U is m.all_users_emb and t.I is m.all_items_emb
    assert (t.n_user, t.n_item) == (5, 2) and t.dev == torch.device("cpu")
    assert isinstance(t, tuple) and t._fields == ("U", "I", "dev", "n_user", "n_item")
