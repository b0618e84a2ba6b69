"""The weight average with two data-parallel ranks, in both multi-rank engines (the set-up of tests/test_ddp_two_ranks_gpu.py:
two processes on the one GPU of the test box over gloo, the persistent decoder kernels and the replay watchdog off for the
reasons given there).  Nothing is exchanged for the average: the parameters are identical on every rank, so the shadows must be,
bit for bit, and each update must be the fp64 `s + rate_t (p_new - s)` of the iteration the engine published."""
import os
import socket
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_IN, T_OUT = 20, 36
DECAY = 0.999


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, graph, out_dir):
    for p in (os.path.join(ROOT, 'tacotron2-vae_amd'), ROOT, os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK='0', HSA_ENABLE_IPC_MODE_LEGACY='0', T2V_TRAIN_PERSISTENT='0', T2V_GRAPH_WATCHDOG='0')
    import torch.distributed as dist
    import distributed as D
    import ema_ref as R
    import hparams as HP
    import t2v_hip
    import train as TR
    from bench import synthetic_batch
    torch.cuda.set_device(0)
    D.init_distributed(backend='gloo', timeout_s=300)
    hp = HP.create_hparams("batch_size=3,anneal_function=constant,distributed_run=True,ema_decay=%r" % DECAY)
    torch.manual_seed(hp.seed + 17 * rank)
    eng = TR.TrainEngine(hp, world_size=world, graph=graph)
    eng.model.vae_gst.eps_override = torch.randn(3, 32, generator=torch.Generator().manual_seed(5 + rank)).cuda()
    opt = eng.optimizer
    res = {'rank': rank, 'graph_ddp': bool(eng.graph_ddp), 'start_equal': bool(torch.equal(opt.ema, opt.params)), 'ratios': []}
    rate = R.rate32(DECAY)
    for it in range(6 if graph else 3):          # (the graph engine captures on the third identical shape)
        batch = synthetic_batch(3, T_IN, T_OUT, 100 + 10 * rank + it, lens_in=[T_IN, T_IN - 3, T_IN - 7],
                                lens_out=[T_OUT, T_OUT - 5, T_OUT - 9])
        s0 = opt.ema.clone()
        eng.step(batch, it)
        torch.cuda.synchronize()
        want, scale = R.ema_ref(s0, opt.params, rate, True, it)
        res['ratios'].append(R.worst_ratio(opt.ema, want, scale))
    t2v_hip.check_async_errors()
    res['n_graphs'] = len(eng._graphs)
    res['differs_from_weights'] = not torch.equal(opt.ema, opt.params)
    for name, arena in (('ema', opt.ema), ('params', opt.params)):
        mine = arena.detach().cpu()
        other = mine.clone()
        D.broadcast(other, 0)
        res[name + '_equal_across_ranks'] = bool(torch.equal(mine.view(torch.int32), other.view(torch.int32)))
    torch.save(res, os.path.join(out_dir, 'r%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('graph', [False, True], ids=['eager_buckets', 'graph_then_reduce_and_step'])
def test_two_ranks_keep_one_shadow(graph, tmp_path):
    import torch.multiprocessing as mp
    import ema_ref as R
    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, graph, str(tmp_path)), nprocs=world, join=True)
    rs = [torch.load(os.path.join(str(tmp_path), 'r%d.pt' % r), weights_only=False) for r in range(world)]
    for r in rs:
        assert r['graph_ddp'] == graph and r['n_graphs'] == (1 if graph else 0)
        assert r['start_equal'] and r['differs_from_weights']
        assert r['params_equal_across_ranks'] and r['ema_equal_across_ranks']
        assert max(r['ratios']) <= R.K_EMA, r['ratios']         # every update at the rate of ITS iteration (9/10, 9/11, ...)
