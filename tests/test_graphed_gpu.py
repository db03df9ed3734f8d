"""hipGraph replay of the inference forward (seoul_tourism_recommendation_ngcf_amd/graphed.py) against the eager forward."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _pkg():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _batch(g, B, U, I, dev):
    r = lambda hi: torch.randint(0, hi, (B,), generator=g).to(dev)  # noqa: E731
    return dict(year=torch.full((B,), 18, device=dev), u_id=r(U), age=r(76), sex=r(2), month=r(13), day=r(32), dow=r(7),
                pos_item=r(I), neg_item=r(I))


@pytest.mark.parametrize("embed,layers", [(65, [64, 64]), (130, [128])])
def test_graphed_forward_replays_the_eager_forward(embed, layers, dev):
    pkg = _pkg()
    slices = pkg.graphs.seoul_standin(dev, seed=5, n_user=700, n_item=40)
    lap = [pkg.graphs.to_sparse_coo(s) for s in slices]
    U, I, B = 700, 40, 96
    num_dict = {"user": U, "item": I, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    torch.manual_seed(3)
    eager = pkg.NGCF(embed, layers, None, None, 0.3, lap, num_dict, B, dev).to(dev).eval()
    graphed_model = copy.deepcopy(eager)
    graphed_model.lap_list = lap
    before = graphed_model.user_embedding.weight.detach().clone()
    fwd = pkg.GraphedForward(graphed_model, B, year_idx=0)
    assert torch.equal(graphed_model.user_embedding.weight.detach(), before)      # capture leaves the weights alone
    g = torch.Generator().manual_seed(11)
    for _ in range(3):                                                            # the injection accumulates over calls
        batch = _batch(g, B, U, I, dev)
        want = eager(node_flag=False, **batch)
        got = fwd(node_flag=False, **batch)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert torch.equal(graphed_model.user_embedding.weight.detach(), eager.user_embedding.weight.detach())
        assert torch.equal(graphed_model.all_items_emb, eager.all_items_emb)
    # eager calls on the SAME module in between (another year slice, a training step that builds the transposed CSR and
    # grows the module's workspace) must not disturb what the captured graph writes through: it owns its buffers
    other = _batch(g, B, U, I, dev)
    other["year"] = torch.full((B,), 19, device=dev)
    for m in (eager, graphed_model):
        m(node_flag=False, **other)
        m.train()
        u, p, n = m(node_flag=False, **other)
        pkg.BPR(0.025, B)(u, p, n).backward()
        m.zero_grad()
        m.eval()
    batch = _batch(g, B, U, I, dev)
    want, got = eager(node_flag=False, **batch), fwd(node_flag=False, **batch)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    bad = _batch(g, B, U, I, dev)
    bad["pos_item"][5] = I                                                        # out of range -> IndexError, like eager
    with pytest.raises(IndexError):
        fwd(node_flag=False, **bad)
    with pytest.raises(IndexError):
        eager(node_flag=False, **bad)                                             # (both have injected the bad batch)
    with pytest.raises(RuntimeError):
        fwd(node_flag=False, **{k: v[:10] for k, v in bad.items()})               # other batch size than captured
    ok = _batch(g, B, U, I, dev)                                                  # usable again after the error
    want, got = eager(node_flag=False, **ok), fwd(node_flag=False, **ok)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_unchanged_callers_get_the_graph_replay(dev):
    """NGCF.forward itself captures and replays (eval mode, torch.no_grad(), node_flag=False): an interleaved sequence of
    evaluation batches (experiment.py:82-91: 25 users, 25 candidate items, no negatives), scoring batches with negatives,
    training steps, a load_state_dict and a second year slice gives bit-identical results on a module with auto_graph on and one
    with it off; replays really happen; a bad id raises within index_check_every calls."""
    pkg = _pkg()
    slices = pkg.graphs.seoul_standin(dev, seed=5, n_user=700, n_item=40)
    lap = [pkg.graphs.to_sparse_coo(s) for s in slices]
    U, I = 700, 40
    num_dict = {"user": U, "item": I, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    torch.manual_seed(3)
    plain = pkg.NGCF(65, [65, 65], 0.3, [0.1, 0.1], 1.0, lap, num_dict, 64, dev).to(dev)
    auto = copy.deepcopy(plain)
    auto.lap_list = lap
    plain.auto_graph = False
    auto.index_check_every = 2
    for m in (plain, auto):
        m.node_dropout_mode = m.mess_dropout_mode = "device"
    g = torch.Generator().manual_seed(11)
    opts = [torch.optim.Adam(m.parameters(), lr=1e-2) for m in (plain, auto)]

    def same(batch):
        outs = []
        for m in (plain, auto):
            m.eval()
            with torch.no_grad():
                outs.append(m(node_flag=False, **batch))
        for a, b in zip(*outs):
            assert a.shape == b.shape and torch.equal(a, b)
        assert torch.equal(plain.user_embedding.weight, auto.user_embedding.weight)
        assert torch.equal(plain.all_items_emb, auto.all_items_emb) and torch.equal(plain.all_users_emb, auto.all_users_emb)
        return outs[1]

    def train_step(batch):
        for m, opt in zip((plain, auto), opts):
            m.train()
            torch.manual_seed(9)
            u, p, n = m(node_flag=True, **batch)
            opt.zero_grad()
            pkg.BPR(0.025, 64)(u, p, n).backward()
            opt.step()

    def eval_batch(year=18):                      # experiment.py:82-91
        b = _batch(g, 25, U, I, dev)
        b["neg_item"] = torch.empty(0)
        b["year"] = torch.full((25,), year, device=dev)
        return b

    held = None
    for it in range(4):
        out = same(eval_batch())
        if it == 2:
            held = (out[0], out[0].clone())
    assert auto._graph_calls >= 2 and len(auto._graphs) == 1           # first call of a shape is eager, the third replays
    assert torch.equal(held[0], held[1])                               # returned tensors are fresh, not the graph's buffers
    assert same(eval_batch())[2].numel() == 0                          # neg_item empty -> torch.empty(0), NGCF.py:153
    for _ in range(3):
        same(_batch(g, 64, U, I, dev))                                 # another shape, with negatives
    assert len(auto._graphs) == 2
    for _ in range(2):
        train_step(_batch(g, 64, U, I, dev))                           # parameters change in place: the graphs stay valid
    calls = auto._graph_calls
    for _ in range(3):
        same(eval_batch())
        same(_batch(g, 64, U, I, dev))
    assert auto._graph_calls == calls + 6 and len(auto._graphs) == 2
    sd = {k: v.clone() + 0.01 for k, v in plain.state_dict().items()}
    for m in (plain, auto):
        m.load_state_dict(sd)
    same(eval_batch())
    for _ in range(3):
        same(eval_batch(year=19))                                      # the other year slice: its own graph
    assert len(auto._graphs) == 3
    for m in (plain, auto):                                            # a replaced parameter with OTHER values: re-capture
        m.user_embedding.weight = torch.nn.Parameter(m.user_embedding.weight.detach() + 0.5)
    for _ in range(3):
        same(eval_batch())
    assert len(auto._graphs) == 3
    bad = eval_batch()
    bad["pos_item"][3] = I
    auto.eval()
    with pytest.raises(IndexError):
        with torch.no_grad():
            for _ in range(3):
                auto(node_flag=False, **bad)
    auto.check_indices_now()                                           # the status word was reset by the raise
    auto.index_check_every = 10 ** 9                                   # r04: no synchronising read at all - the pinned mirror reports it
    good = eval_batch()
    with torch.no_grad():
        for _ in range(3):
            auto(node_flag=False, **good)                              # (this shape replays)
        auto(node_flag=False, **bad)                                   # no raise: nothing has read the word yet
        torch.cuda.synchronize()
        with pytest.raises(IndexError):
            auto(node_flag=False, **good)
        auto(node_flag=False, **good)
    auto.index_check_every = 2
    plain.user_embedding.weight.data.copy_(auto.user_embedding.weight.data)
    plain.invalidate_all_E()       # r04: a write through .data from outside bypasses the version counter the retained all_E watches
    same(eval_batch())
    # r04: a caller that KEEPS model.all_items_emb (demo.py:233 reads it) keeps what it read - the reference hands out a fresh all_E per
    # call (NGCF.py:147-149).  Under replays the attribute is a view of the graph's static buffer: while somebody holds it (or a slice
    # of it) the forward runs eagerly into fresh tensors; replays resume when it is released.
    b1, b2, b3 = eval_batch(), eval_batch(), eval_batch()
    same(b1)
    same(b1)
    calls = auto._graph_calls
    held = auto.all_items_emb
    kept = held.clone()
    same(b2)                                                            # another batch: the injected rows (and so all_E) change
    assert torch.equal(held, kept) and not torch.equal(auto.all_items_emb, kept) and auto._graph_calls == calls
    piece = auto.all_users_emb[3:9]                                     # (an eager result now; hold a slice of it and release the first)
    del held
    same(b3)
    del piece
    same(b1)
    same(b2)
    assert auto._graph_calls > calls                                    # replaying again
    held = auto.all_users_emb[:5]                                       # a SLICE of a replayed result
    kept = held.clone()
    calls = auto._graph_calls
    same(b3)
    assert torch.equal(held, kept) and auto._graph_calls == calls
    del held


def test_graphed_train_step_replays_the_eager_step(dev):
    """GraphedTrainStep (forward with node + message dropout in device mode, BPR, backward, Adam) against the same steps issued
    eagerly: same seed, same batches -> the same losses and the same parameters bit for bit, step after step (the dropout seeds live
    in device memory and are stepped inside the graph, so every replay draws the masks the eager step would)."""
    pkg = _pkg()
    slices = pkg.graphs.seoul_standin(dev, seed=5, n_user=700, n_item=40)
    lap = [pkg.graphs.to_sparse_coo(s) for s in slices]
    U, I, B = 700, 40, 128
    num_dict = {"user": U, "item": I, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    g = torch.Generator().manual_seed(21)
    batches = [_batch(g, B, U, I, dev) for _ in range(7)]
    for b in batches:
        b["u_id"][:9] = b["u_id"][9:18]                               # duplicates in every batch
    results = []
    for graphed in (False, True):
        torch.manual_seed(3)
        model = pkg.NGCF(65, [65, 65, 65], 0.3, [0.1, 0.1, 0.1], 1.0, lap, num_dict, B, dev).to(dev)
        model.train()
        model.node_dropout_mode = model.mess_dropout_mode = "device"
        opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)
        crit = pkg.BPR(0.025, B)
        torch.manual_seed(11)                                          # the module's seed chain follows torch.manual_seed
        losses = []
        if graphed:
            step = pkg.GraphedTrainStep(model, crit, opt, batches[0], node_flag=True, warmup=3)
            for b in batches[1:]:
                losses.append(float(step(**b)))
        else:
            for b in [batches[0]] * 3 + batches[1:]:
                u, p, n = model(node_flag=True, **b)
                opt.zero_grad()
                loss = crit(u, p, n)
                loss.backward()
                opt.step()
                losses.append(float(loss))
            losses = losses[3:]
        results.append((losses, {k: v.detach().clone() for k, v in model.state_dict().items()}))
    assert results[0][0] == results[1][0], (results[0][0], results[1][0])
    assert len(set(results[0][0])) > 1                                 # the losses move: new masks and new parameters every step
    for k in results[0][1]:
        assert torch.equal(results[0][1][k], results[1][1][k]), k
    with pytest.raises(RuntimeError, match="capturable"):
        pkg.GraphedTrainStep(model, crit, torch.optim.Adam(model.parameters(), lr=1e-2), batches[0])


def test_unchanged_training_loops_get_graph_replays(dev):
    """NGCF.auto_train_graph: a plain training loop (experiment.py:45-58: forward, zero_grad, BPR, backward, Adam.step) in device
    dropout mode.  From the second call of a shape on, forward and backward are replays of two captured graphs; the run must be the
    eager run bit for bit - losses and every parameter after every step - over two batch shapes (full batches and a shorter last
    batch of an epoch), and an out-of-range id must still raise."""
    pkg = _pkg()
    slices = pkg.graphs.seoul_standin(dev, seed=6, n_user=600, n_item=30)
    lap = [pkg.graphs.to_sparse_coo(s) for s in slices]
    U, I, B = 600, 30, 96
    num_dict = {"user": U, "item": I, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    g = torch.Generator().manual_seed(31)
    epoch = lambda: [_batch(g, B, U, I, dev) for _ in range(3)] + [_batch(g, 40, U, I, dev)]   # noqa: E731
    batches = epoch() + epoch() + epoch()
    for b in batches:
        b["u_id"][:5] = b["u_id"][5:10]                               # duplicates in every batch
    results = []
    for auto in (False, True):
        torch.manual_seed(4)
        model = pkg.NGCF(65, [65, 65, 65], 0.3, [0.1, 0.1, 0.1], 1.0, lap, num_dict, B, dev).to(dev)
        model.train()
        model.node_dropout_mode = model.mess_dropout_mode = "device"
        model.auto_train_graph = auto
        opt = torch.optim.Adam(model.parameters(), lr=1e-2)
        crit = pkg.BPR(0.025, B)
        torch.manual_seed(12)
        losses, states = [], []
        for b in batches:
            u, p, n = model(node_flag=True, **b)
            opt.zero_grad()
            loss = crit(u, p, n)
            loss.backward()
            opt.step()
            losses.append(float(loss))
            states.append(model.w1_list[0].weight.detach().clone())
        results.append((losses, states, {k: v.detach().clone() for k, v in model.state_dict().items()}))
        assert len(model._train_graphs) == (2 if auto else 0)          # one pair of graphs per batch shape
    assert results[0][0] == results[1][0], (results[0][0], results[1][0])
    assert len(set(results[0][0])) > 1
    for a, b_ in zip(results[0][1], results[1][1]):
        assert torch.equal(a, b_)
    for k in results[0][2]:
        assert torch.equal(results[0][2][k], results[1][2][k]), k
    # the last model replays graphs: a bad id is reported (sticky status word, read every index_check_every-th call)
    model.index_check_every = 1
    bad = {k: v.clone() for k, v in batches[0].items()}
    bad["pos_item"][3] = I + 5
    with pytest.raises(IndexError):
        model(node_flag=True, **bad)
    u, p, n = model(node_flag=True, **batches[0])                      # and the model keeps working
    assert torch.isfinite(u).all()
    # r04: without any synchronising read (index_check_every far away) the bad id of a replay is reported by the NEXT call that
    # finds the GPU past it - the replay's last node copies the sticky status word into pinned host memory
    model.index_check_every = 10 ** 9
    del u, p, n                                                        # (a forward whose backward can still run keeps the next one eager)
    model(node_flag=True, **bad)                                       # no raise here: nothing has read the word
    torch.cuda.synchronize()                                           # (a training loop gets here through loss.item(), a log line, ...)
    with pytest.raises(IndexError):
        model(node_flag=True, **batches[0])
    assert torch.isfinite(model(node_flag=True, **batches[0])[0]).all()
    model.index_check_every = 1
    # eval-mode calls in between take the inference path and do not disturb the training graphs
    model.eval()
    with torch.no_grad():
        model(node_flag=False, **batches[1])
    model.train()
    u2, p2, n2 = model(node_flag=True, **batches[1])
    assert u2.requires_grad and torch.isfinite(u2).all()
    # gradient accumulation over two backward calls without zero_grad, and zero_grad(set_to_none=False): the graph's gradient
    # buffers must not be what `.grad` accumulates into.  Without dropout the same batch gives the same gradient bit for bit.
    torch.manual_seed(5)
    m2 = pkg.NGCF(65, [65, 65], None, None, 1.0, lap, num_dict, B, dev).to(dev)
    m2.train()
    m2.node_dropout_mode = m2.mess_dropout_mode = "device"
    w = m2.w1_list[0].weight
    grads = []
    for it in range(4):                                                # calls 0 (eager), 1 (captures), 2, 3 (replays)
        m2.zero_grad()
        u, p, n = m2(node_flag=False, **batches[0])
        crit(u, p, n).backward()
        grads.append(w.grad.clone())
    assert len(m2._train_graphs) == 1 and all(torch.equal(grads[0], g_) for g_ in grads[1:])
    u, p, n = m2(node_flag=False, **batches[0])                        # no zero_grad: accumulate
    crit(u, p, n).backward()
    assert torch.equal(w.grad, grads[0] + grads[0])
    for q in m2.parameters():                                          # zero in place, keep the tensors
        if q.grad is not None:
            q.grad.zero_()
    u, p, n = m2(node_flag=False, **batches[0])
    crit(u, p, n).backward()
    assert torch.equal(w.grad, grads[0])
    assert torch.equal(m2.user_embedding.weight.grad[batches[0]["u_id"][0]], m2.user_embedding.weight.grad[batches[0]["u_id"][0]])
