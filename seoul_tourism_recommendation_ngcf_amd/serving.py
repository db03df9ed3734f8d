"""The scaffold under the model-level entry points of `evaluate.py` and `recommend.py`: eval mode under no_grad with the caller's mode
handed back, one propagate and its two tables, the id default, the chunk loop, one device status word and ONE read-back at the end.
It launches nothing of its own; it arranges calls the entry points make.  (The feature injection and its cache touch are the
model's: `NGCF._inject_features`.)"""
import contextlib
from collections import namedtuple

import torch

from . import engine


@contextlib.contextmanager
def inference(model):
    """`model` in eval mode under `torch.no_grad()`; the caller's mode is restored on exit, also when the body raises."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        model.train(was_training)


Tables = namedtuple("Tables", "U I dev n_user n_item")                 # U, I: strided views of all_E, no copies


def propagated(model, year_idx) -> Tables:
    """`model.propagate(year_idx)` and the tables it leaves on the model."""
    model.propagate(year_idx)
    U, I = model.all_users_emb, model.all_items_emb  # noqa: E741
    return Tables(U, I, U.device, int(U.shape[0]), int(I.shape[0]))


def as_sets(s, t: Tables) -> "engine.ItemSets":
    """An engine.ItemSets as it is; (users, items[, weights]) pairs as the ItemSets over `t`'s rows."""
    return s if isinstance(s, engine.ItemSets) else engine.ItemSets.from_pairs(s[0].to(t.dev), s[1].to(t.dev), t.n_user, t.n_item)


def ids_or_all(users, n, dev) -> torch.Tensor:
    """`users` as a flat int64 vector on `dev`; None means all of [0, n)."""
    users = torch.arange(n, device=dev, dtype=torch.int64) if users is None else users
    return users.reshape(-1).to(device=dev, dtype=torch.int64)


def chunks(n, size):
    """The slices of [0, n) in order, `size` entries each and the last one what is left."""
    n, size = int(n), int(size)
    return (slice(c0, min(c0 + size, n)) for c0 in range(0, n, size))


def status_word(dev) -> torch.Tensor:
    """The call's sticky device status word: its launches OR into it, `read_back` reads it, once."""
    return torch.zeros(1, dtype=torch.int32, device=dev)


def read_back(status, *vectors):
    """The call's one device-to-host transfer: (status word, `vectors` on the host as one); the word travels in their dtype."""
    if not vectors:
        return int(status.item()), None
    host = torch.cat((*vectors, status.to(vectors[0].dtype))).cpu()
    return int(host[-1]), host[:-1]


def year_slice(model, year):
    """(Laplacian slice, years on the host - a device tensor costs one read-back here): (0, None) for None, (`model._year_index`
    of it, [1] vector) for one year, (None, [n] vector) for any other count: the caller refuses that or groups by it."""
    if year is None:
        return 0, None
    year_h = torch.as_tensor(year).reshape(-1).cpu()
    return (model._year_index(year_h) if int(year_h.numel()) == 1 else None), year_h
