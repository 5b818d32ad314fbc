"""Two ranks running the REAL GaussILRMA through `distributed.separate_sharded` (the config-5 driver).

With >= 2 GPUs: one process per GPU, backend "nccl" (= RCCL over xGMI), edge buffers in HBM.  With one GPU (the
gpurun box): the same two processes share cuda:0 and stage the scatter/gather through host memory over "gloo" --
everything but the transport is identical.  Either way the sharded result must equal the single-process batched
result BIT FOR BIT, in the original utterance order, for an even and a ragged split."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

M, F, T, K, ITER = 4, 33, 96, 4, 4


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run_workers(target, args_for_rank, world=2, timeout=600):
    """Start `world` spawned processes, collect one queue item per rank, always reap the children."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=args_for_rank(r, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        results = sorted([q.get(timeout=timeout) for _ in range(world)], key=lambda r: r[0])
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
        return results
    finally:
        for p in procs:  # a hung collective must not outlive the test
            if p.is_alive():
                p.terminate()
                p.join(timeout=30)


def _mixtures(n_items):
    rng = np.random.default_rng(11)
    S = (rng.standard_normal((n_items, M, F, T)) + 1j * rng.standard_normal((n_items, M, F, T))) * \
        rng.random((n_items, M, 1, T)) ** 2
    A = rng.standard_normal((n_items, F, M, M)) + 1j * rng.standard_normal((n_items, F, M, M))
    return np.einsum("bfmn,bnft->bmft", A, S)


def _init_fn(model, lo, hi):
    st = [np.random.RandomState(111 + u) for u in range(lo, hi)]
    model.basis = np.stack([s.rand(M, F, K) for s in st])
    model.activation = np.stack([s.rand(M, K, T) for s in st])


def _factory():
    from audio_source_separation_amd.bss.ilrma import GaussILRMA
    return GaussILRMA(n_basis=K, recordable_loss=True)


def _worker(rank, world, port, n_items, backend, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank if backend == "nccl" else 0),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    sys.path.insert(0, ROOT)
    from audio_source_separation_amd import distributed as D
    D.init_from_env(backend=backend)
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    comm_dev = dev if backend == "nccl" else "cpu"
    x_all = torch.from_numpy(_mixtures(n_items)).to(comm_dev) if rank == 0 else None
    y, model = D.separate_sharded(_factory, x_all, n_items, (M, F, T), torch.complex128, dev, iteration=ITER,
                                  init_fn=_init_fn, comm_device=comm_dev)
    lo, hi = D.shard_range(n_items, world, rank)
    loss = np.asarray(model.loss) if hi > lo else None  # (ITER+1, n_local)
    tmax = D.max_over_ranks(1.0 + rank, device=comm_dev)
    D.barrier(dev)
    q.put((rank, None if y is None else y.cpu().numpy(), loss, tmax))
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("n_items", [4, 5])
def test_two_ranks_real_gauss_ilrma_bit_identical(n_items):
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    world = 2
    port = _free_port()
    results = _run_workers(_worker, lambda r, q: (r, world, port, n_items, backend, q), world)
    y = results[0][1]
    assert results[1][1] is None and results[0][3] == 2.0 and results[1][3] == 2.0
    # single process, all utterances in one batched call
    single = _factory()
    _init_fn(single, 0, n_items)
    ref = single(_mixtures(n_items), iteration=ITER)
    assert y.shape == ref.shape and np.array_equal(y, ref)
    loss = np.concatenate([r[2] for r in results if r[2] is not None], axis=1)
    assert np.array_equal(loss, np.asarray(single.loss))


def test_rccl_single_rank_group_and_bench_under_launcher():
    """RCCL itself on this box: a 1-rank "nccl" group (all-reduce, barrier), then bench.py under torch.distributed.run
    exactly as the driver launches it (rendezvous on 127.0.0.1), with the config-5 leg on a reduced batch."""
    code = (
        "import os, torch, torch.distributed as dist\n"
        "os.environ.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT='%d')\n"
        "torch.cuda.set_device(0)\n"
        "dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))\n"
        "t = torch.ones(4, device='cuda', dtype=torch.float64)\n"
        "dist.all_reduce(t); dist.barrier(device_ids=[0]); torch.cuda.synchronize()\n"
        "assert t.sum().item() == 4.0\n"
        "dist.destroy_process_group(); print('rccl ok')\n" % _free_port())
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "rccl ok" in r.stdout, r.stderr[-2000:]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--full", "--steps",
           "3", "--warmup", "1", "--bins", "129", "--frames", "512", "--cpu-iters", "0", "--kernel-reps", "3",
           "--roofline-b8", "2", "--config5", "on", "--config5-utterances", "3", "--config5-iterations", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    import json
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 1 and out["value"] > 0 and out["roofline"]["frac"] > 0
    assert out["roofline_b8"]["utterances_per_launch"] == 2
    assert out["config5"]["utterances"] == 3 and out["config5"]["outputs_finite"] and out["config5"]["value"] > 0


def test_cabi_comm_edges_on_a_one_rank_communicator():
    """The multi-GPU edges through the C-ABI (include/assx.h: assx_comm_unique_id / assx_comm_init / assx_scatter /
    assx_gather; round 5's review, missing #3: a non-Python host had no multi-GPU path).  What one GPU can run of it: a 1-rank
    RCCL communicator made through the library (librccl.so loaded on first use), whose root sends its block to and receives it
    from ITSELF inside the same grouped ncclSend / ncclRecv batch that root <-> 7 peers use -- complex128 and complex64, 5 ragged
    utterances, a non-default stream; received blocks bit-identical, and the aliasing case (the block already in place) moves
    nothing.  In its own interpreter: RCCL initialises process-wide state."""
    code = (
        "import sys, torch\n"
        "sys.path.insert(0, %r)\n"
        "from audio_source_separation_amd import comm as C\n"
        "dev = torch.device('cuda', 0)\n"
        "assert C.shard_range(64, 8, 3) == (24, 32) and C.shard_range(13, 8, 7) == (12, 13)\n"
        "cm = C.Comm(1, 0, C.unique_id(), device=dev)\n"
        "g = torch.Generator(device=dev).manual_seed(3)\n"
        "for dt, rt in ((torch.complex128, torch.float64), (torch.complex64, torch.float32)):\n"
        "    x = torch.view_as_complex(torch.randn((5, 4, 9, 20, 2), dtype=rt, device=dev, generator=g))\n"
        "    st = torch.cuda.Stream(device=dev)\n"
        "    with torch.cuda.stream(st):\n"
        "        loc = cm.scatter(x, 5, (4, 9, 20), dt)\n"
        "        back = cm.gather(loc * 2, 5)\n"
        "    st.synchronize()\n"
        "    assert loc.data_ptr() != x.data_ptr() and torch.equal(loc, x) and torch.equal(back, x * 2)\n"
        "cm.close()\n"
        "from audio_source_separation_amd._lib import AssxError\n"
        "for world, rank in ((2, 5), (0, 0), (3, -1)):\n"
        "    try:\n"
        "        C.Comm(world, rank, C.unique_id(), device=dev)\n"
        "        raise SystemExit('bad world / rank %%d / %%d accepted' %% (world, rank))\n"
        "    except AssxError as e:\n"
        "        assert 'bad world / rank' in str(e), e\n"
        "print('cabi comm ok')\n" % ROOT)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "cabi comm ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_rccl_grouped_send_recv_on_views_of_a_complex_array():
    """The edge traffic of config 5 through RCCL itself, on what one GPU can run: a 1-rank "nccl" group whose rank sends
    to and receives from ITSELF inside one grouped batch (ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd -- the
    call sequence `scatter_utterances` / `gather_utterances` issue towards 7 peers), on exactly the operands those
    functions build: `view_as_real` views of contiguous row blocks of a complex array at non-zero storage offsets, for a
    ragged partition, complex128 and complex64.  Received blocks must equal the sent ones bit for bit, and the rest of
    the destination must stay untouched.  (More than one rank over xGMI needs more than one GPU: the driver's run.)"""
    code = (
        "import os, sys, torch, torch.distributed as dist\n"
        "sys.path.insert(0, %r)\n"
        "os.environ.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT='%d')\n"
        "from audio_source_separation_amd import distributed as D\n"
        "torch.cuda.set_device(0)\n"
        "dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))\n"
        "dev = torch.device('cuda', 0)\n"
        "for dt in (torch.complex128, torch.complex64):\n"
        "    g = torch.Generator(device=dev).manual_seed(5)\n"
        "    x = torch.view_as_complex(torch.randn((13, 4, 9, 40, 2), dtype=torch.float64, device=dev, generator=g)).to(dt)\n"
        "    out = torch.full_like(x, 7.0)\n"
        "    ops, blocks = [], []\n"
        "    for r in range(1, 8):  # the blocks of peers 1..7 of an 8-way partition of 13 utterances (ragged)\n"
        "        a, b = D.shard_range(13, 8, r)\n"
        "        s, d = D._as_real(x[a:b]), D._as_real(out[a:b])\n"
        "        assert s.is_contiguous() and d.is_contiguous() and s.storage_offset() > 0 and s.dtype == x.real.dtype\n"
        "        ops += [dist.P2POp(dist.isend, s, 0), dist.P2POp(dist.irecv, d, 0)]\n"
        "        blocks.append((a, b))\n"
        "    D._run_p2p(ops)\n"
        "    torch.cuda.synchronize()\n"
        "    a0, b0 = D.shard_range(13, 8, 0)\n"
        "    assert torch.equal(out[b0:], x[b0:]) and bool((out[a0:b0] == 7.0).all())\n"
        "    # the library functions themselves on a 1-rank group\n"
        "    xl = D.scatter_utterances(x, 13, (4, 9, 40), dt, dev)\n"
        "    assert torch.equal(D.gather_utterances(xl, 13), x)\n"
        "assert D.max_over_ranks(3.5, device=dev) == 3.5\n"
        "D.barrier(dev); dist.destroy_process_group(); print('edges ok')\n" % (ROOT, _free_port()))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "edges ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------------------
# F-sharded single utterance with the HIP shard ops (bss/ilrma_fshard.py)
# ---------------------------------------------------------------------------------------------------------------
def _fs_problem(Mx, Fx, Tx, Kx, seed=31):
    rng = np.random.default_rng(seed)
    S = (rng.standard_normal((Mx, Fx, Tx)) + 1j * rng.standard_normal((Mx, Fx, Tx))) * (0.1 + rng.random((Mx, 1, Tx)) ** 2)
    A = rng.standard_normal((Fx, Mx, Mx)) + 1j * rng.standard_normal((Fx, Mx, Mx))
    st = np.random.RandomState(seed)
    return np.einsum("fmn,nft->mft", A, S), st.rand(Mx, Fx, Kx), st.rand(Mx, Kx, Tx)


@pytest.mark.parametrize("Mx,Kx,domain,normalize,dtype", [(4, 4, 2, "power", "float64"), (3, 10, 1, "power", "float64"),
                                                          (2, 3, 2, False, "float64"), (5, 3, 2, "power", "float64"),
                                                          (4, 4, 2, "power", "float32")])
def test_frequency_sharded_ilrma_matches_oracle_and_class(Mx, Kx, domain, normalize, dtype):
    """1, 2 and 3 bin shards on one process: each equals the oracle's (and the GaussILRMA class's) unsharded result
    up to the rounding of the f-reduction; ragged shards (F = 23); the loss list has iteration + 1 entries."""
    from audio_source_separation_amd.bss.ilrma import GaussILRMA
    from audio_source_separation_amd.bss.ilrma_fshard import FrequencyShardedGaussILRMA
    from oracle import oracle_np as orc
    Fx, Tx = 23, 200
    X, T0, V0 = _fs_problem(Mx, Fx, Tx, Kx)
    ref = orc.gauss_ilrma(X, 4, T0, V0, domain=domain, normalize=normalize)
    tolW, tolL = (1e-8, 1e-10) if dtype == "float64" else (2e-2, 1e-4)
    for S in (1, 2, 3):
        m = FrequencyShardedGaussILRMA(n_basis=Kx, domain=domain, normalize=normalize, n_shards=S, dtype=dtype)
        Y = m(X, iteration=4, basis=T0, activation=V0)
        assert Y.shape == X.shape and Y.dtype == np.complex128 and len(m.loss) == 5
        assert np.linalg.norm(m.demix_filter - ref["W"]) / np.linalg.norm(ref["W"]) < tolW
        assert np.linalg.norm(Y - ref["Y"]) / np.linalg.norm(ref["Y"]) < tolW
        assert np.linalg.norm(m.basis - ref["T"]) / np.linalg.norm(ref["T"]) < tolW
        assert np.linalg.norm(m.activation - ref["V"]) / np.linalg.norm(ref["V"]) < tolW
        np.testing.assert_allclose(m.loss, ref["loss"], rtol=tolL)
    if dtype == "float64":
        g = GaussILRMA(n_basis=Kx, domain=domain, normalize=normalize)
        g.basis, g.activation = T0, V0
        Yg = g(X, iteration=4)
        assert np.linalg.norm(Y - Yg) / np.linalg.norm(Yg) < 1e-8


@pytest.mark.parametrize("spatial,normalize", [("ISS", "power"), ("IP2", "power"), ("IP", "projection-back"),
                                               ("ISS", "projection-back"), ("IP2", False)])
def test_frequency_sharded_other_sweeps_and_projection_back(spatial, normalize):
    """The F-sharded mode beyond IP + 'power' (ilrma.py:313-330, 537-646): ISS and IP2 sweeps and the projection-back
    normalisation are per bin, so a shard runs them unchanged; 1 and 3 ragged shards against the oracle's unsharded
    run (IP2: the pair sequence and the pair-restricted source model included)."""
    from audio_source_separation_amd.bss.ilrma_fshard import FrequencyShardedGaussILRMA
    from oracle import oracle_np as orc
    Mx, Fx, Tx, Kx, iters = 4, 23, 200, 3, 5
    X, T0, V0 = _fs_problem(Mx, Fx, Tx, Kx, seed=37)
    if spatial == "ISS":
        ref = orc.gauss_ilrma_iss(X, iters, T0, V0, normalize=normalize)
    elif spatial == "IP2":
        ref = orc.gauss_ilrma_ip2(X, iters, T0, V0, normalize=normalize)
    else:
        ref = orc.gauss_ilrma(X, iters, T0, V0, normalize=normalize)
    for S in (1, 3):
        m = FrequencyShardedGaussILRMA(n_basis=Kx, normalize=normalize, algorithm_spatial=spatial, n_shards=S)
        Y = m(X, iteration=iters, basis=T0, activation=V0)
        assert np.linalg.norm(Y - ref["Y"]) / np.linalg.norm(ref["Y"]) < 1e-7
        assert np.linalg.norm(m.basis - ref["T"]) / np.linalg.norm(ref["T"]) < 1e-7
        assert np.linalg.norm(m.activation - ref["V"]) / np.linalg.norm(ref["V"]) < 1e-7
        np.testing.assert_allclose(m.loss, ref["loss"], rtol=1e-9)


def _fs_worker(rank, world, port, backend, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank if backend == "nccl" else 0),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    sys.path.insert(0, ROOT)
    from audio_source_separation_amd import distributed as D
    from audio_source_separation_amd.bss.ilrma_fshard import FrequencyShardedGaussILRMA
    D.init_from_env(backend=backend)
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    X, T0, V0 = _fs_problem(4, 23, 200, 4)
    m = FrequencyShardedGaussILRMA(n_basis=4, n_shards=4, device=dev, comm_device=dev if backend == "nccl" else "cpu")
    Y = m(X, iteration=3, basis=T0, activation=V0)
    out = (rank, Y, np.asarray(m.loss), m.demix_filter, m.basis, m.activation)
    D.barrier(dev)
    q.put(out)
    torch.distributed.destroy_process_group()


def test_frequency_sharded_ilrma_two_ranks_bitwise():
    """4 bin shards over 2 ranks (2 shards each) == the same 4 shards on one process, bit for bit on every rank."""
    from audio_source_separation_amd.bss.ilrma_fshard import FrequencyShardedGaussILRMA
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    world = 2
    port = _free_port()
    results = _run_workers(_fs_worker, lambda r, q: (r, world, port, backend, q), world)
    X, T0, V0 = _fs_problem(4, 23, 200, 4)
    m = FrequencyShardedGaussILRMA(n_basis=4, n_shards=4)
    Y = m(X, iteration=3, basis=T0, activation=V0)
    single = (Y, np.asarray(m.loss), m.demix_filter, m.basis, m.activation)
    for res in results:
        for a, b in zip(res[1:], single):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("world,n_utt", [(2, 5), (8, 13)])
def test_bench_n_ranks_whole_flow_on_one_gpu(world, n_utt):
    """`python bench.py --gpus N` end to end -- self-launch under torch.distributed.run, the weak-scaling headline
    line, the config-5 leg with a ragged batch and real scatter / gather edges -- with every rank on cuda:0 and the edges
    staged over gloo (the test-only --comm-backend gloo --share-gpu mode; RCCL needs one GPU per rank).  Everything but
    the transport is what the driver's 8-GPU run executes; N = 8 is that run's process layout (round 5's review, item 4)."""
    import json
    from audio_source_separation_amd import distributed as D
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--full", "--comm-backend", "gloo",
           "--share-gpu", "--steps", "3", "--warmup", "1", "--bins", "129", "--frames", "512", "--cpu-iters", "0", "--kernel-reps", "3",
           "--roofline-b8", "2", "--config5-utterances", str(n_utt), "--config5-iterations", "2", "--prewarm-ms", "5"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1  # ONE JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == world
    assert out["comm"] == {"backend": "gloo", "world_size": world, "utterances_per_rank": [1] * world}
    assert out["value"] > 0 and out["scaling"] == "weak" and out["cpu_baseline"] is None
    c5 = out["config5"]
    assert c5["utterances"] == n_utt and c5["utterances_per_gpu"] == D.shard_sizes(n_utt, world) and c5["outputs_finite"]
    assert sum(c5["utterances_per_gpu"]) == n_utt and max(c5["utterances_per_gpu"]) - min(c5["utterances_per_gpu"]) <= 1
    assert c5["value"] >= c5["value_incl_edges"] > 0 and c5["seconds_scatter"] > 0 and c5["seconds_gather"] > 0


# ------------------------------------------------------------------------------------------
# Launch order of a batched pass (csrc/assx_stream.hpp: workgroup_range): utterance-sequential with alternating
# direction (default) against the first XCD-aware order (ASSX_UTT_ORDER=0).  The switch is read once per process,
# so each order runs in its own interpreter; the order decides when a range runs, never what it computes.
# ------------------------------------------------------------------------------------------
_ORDER_CODE = r"""
import hashlib, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from audio_source_separation_amd.bss.ilrma import GaussILRMA
from audio_source_separation_amd.bss.iva import AuxLaplaceIVA
rng = np.random.default_rng(5)
B, M, F, T, K = 3, 4, 37, 300, %(K)d
X = rng.standard_normal((B, M, F, T)) + 1j * rng.standard_normal((B, M, F, T))
h = hashlib.sha1()
for cls, kw in ((GaussILRMA, dict(n_basis=K)), (AuxLaplaceIVA, {})):
    np.random.seed(3)
    m = cls(dtype=%(dtype)r, **kw)
    Y = m(torch.from_numpy(X).to("cuda:0"), iteration=5)      # odd number of passes: both directions, both parities
    h.update(np.ascontiguousarray(Y.cpu().numpy()).tobytes())
    h.update(np.ascontiguousarray(np.asarray(m.demix_filter)).tobytes())
    h.update(np.asarray(m.loss, dtype=np.float64).tobytes())
print("DIGEST", h.hexdigest())
"""


@pytest.mark.parametrize("dtype,K,forced_g", [("float64", 4, 0), ("float64", 4, 5), ("float32", 4, 11), ("float64", 10, 0)])
def test_batched_launch_orders_give_the_same_bits(dtype, K, forced_g):
    # the legacy order exists in laboratory builds only; in the shipped library "the order never changes a result" is pinned
    # by batched == single bit for bit (tests/test_gpu_fullsize.py::test_config5_batch_of_8_full_size_equals_single and the
    # batched cases of tests/test_gpu_ops.py: a single utterance has no utterance order)
    from conftest import need_lab
    need_lab("ASSX_UTT_ORDER")
    digests = []
    for order in ("1", "0"):
        env = dict(os.environ, ASSX_UTT_ORDER=order, HSA_ENABLE_IPC_MODE_LEGACY="0")
        if forced_g:
            env["ASSX_G"] = str(forced_g)  # a handful of long ranges per utterance: padding slots, ragged eighths
        else:
            env.pop("ASSX_G", None)
        r = subprocess.run([sys.executable, "-c", _ORDER_CODE % dict(root=ROOT, dtype=dtype, K=K)], capture_output=True,
                           text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        digests.append([ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][-1])
    assert digests[0] == digests[1]
