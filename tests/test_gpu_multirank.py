"""The multi-rank code paths of the registration with MORE THAN ONE rank:

  * callback all-reduce (kicp_reg_set_allreduce): 2 and 3 processes share device 0; every iteration the pass kernel leaves its
    24 limb words in HBM, the callback sums them across the processes (through torch.distributed / gloo on the host - what
    matters here is the DEVICE side: totals left for a collective, all-reduce on the registration's stream, k_publish_words
    / the separate solve kernel afterwards), and every rank must return the single-process bits;
  * built-in RCCL communicator (kicp_reg_comm_init) with two ranks on two GPUs - RCCL refuses two ranks on one device, so this
    one needs a box with >= 2 GPUs and is skipped elsewhere;
  * bench.py itself launched by torch.distributed.run with two ranks (host shared segment, gloo process group, both ranks on
    device 0): the launch path the driver uses for its scaling runs must at least work end to end.
"""
import json
import multiprocessing as mp
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "registration_small.npz")
CASES = ("a", "b", "c")


def _single_process_results():
    import kinematic_icp_amd as K
    g = np.load(GOLD)
    single, out = K.KinematicRegistration(), []
    for case in CASES:
        m = K.VoxelHashMap(float(g[case + "_voxel"]), float(g[case + "_maxrange"]), 20)
        m.AddPoints(g[case + "_map"])
        pose = single.ComputeRobotMotion(g[case + "_frame"], m, g[case + "_last"], g[case + "_rel"], float(g[case + "_tau"]))
        assert single.last_stats.iterations == int(g[case + "_iters"])
        out.append((pose, single.last_stats.iterations))
    return out


def _run_cases(reg, world, rank):
    import kinematic_icp_amd as K
    from kinematic_icp_amd import sharding as sh
    g = np.load(GOLD)
    out = []
    for case in CASES:
        m = K.VoxelHashMap(float(g[case + "_voxel"]), float(g[case + "_maxrange"]), 20)
        m.AddPoints(g[case + "_map"])
        frame = g[case + "_frame"]
        lo, hi = sh.shard_bounds(len(frame), world, rank)
        pose = reg.ComputeRobotMotion(K.DeviceFrame(frame[lo:hi], device=reg.device), m, g[case + "_last"], g[case + "_rel"], float(g[case + "_tau"]))
        out.append((pose, reg.last_stats.iterations))
    return out


def _callback_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    try:
        import torch
        import torch.distributed as dist
        import kinematic_icp_amd as K
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group(backend="gloo")
        torch.cuda.set_device(0)
        reg = K.KinematicRegistration(device=0)
        calls = []

        def allreduce(ptr, count, stream):
            class _Arr:
                __cuda_array_interface__ = {"shape": (count,), "typestr": "<i8", "data": (ptr, False), "version": 2}
            ext = torch.cuda.ExternalStream(stream)
            with torch.cuda.stream(ext):
                t = torch.as_tensor(_Arr(), device="cuda")
                host = t.cpu()                       # ordered behind the pass kernel on the registration's stream
                dist.all_reduce(host, op=dist.ReduceOp.SUM)
                t.copy_(host)                        # and back, before the publish / solve kernel that follows
                ext.synchronize()
            calls.append(count)

        reg.set_allreduce(allreduce)
        out = _run_cases(reg, world, rank)
        assert calls and all(c == 24 for c in calls)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, out, None))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, [], repr(e) + "\n" + traceback.format_exc()))


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _spawn(target, world, extra):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world) + extra + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(world):
        rank, out, err = q.get(timeout=300)
        assert err is None, "rank %d: %s" % (rank, err)
        results[rank] = out
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return results


@pytest.mark.parametrize("world", [2, 3])
def test_callback_allreduce_across_processes(world):
    results = _spawn(_callback_worker, world, (_free_port(),))
    ref = _single_process_results()
    for r in range(world):
        for (pose, iters), (pose1, iters1) in zip(results[r], ref):
            assert iters == iters1
            assert np.array_equal(pose, pose1)  # exact integer sums, the same host-side solve: the same bits


def _rccl_worker(rank, world, uid, q):
    sys.path.insert(0, ROOT)
    try:
        import kinematic_icp_amd as K
        reg = K.KinematicRegistration(device=rank)
        reg.comm_init(world, rank, uid)
        out = _run_cases(reg, world, rank)
        reg.comm_destroy()
        q.put((rank, out, None))
    except Exception as e:  # noqa: BLE001
        q.put((rank, [], repr(e)))


def test_rccl_allreduce_two_gpus():
    import kinematic_icp_amd as K
    if K.device_count() < 2:
        pytest.skip("needs two GPUs: RCCL does not accept two ranks on one device")
    results = _spawn(_rccl_worker, 2, (K.comm_unique_id(),))
    ref = _single_process_results()
    for r in range(2):
        for (pose, iters), (pose1, iters1) in zip(results[r], ref):
            assert iters == iters1 and np.array_equal(pose, pose1)


def test_bench_launch_path_with_two_ranks_on_one_gpu():
    """bench.py under torch.distributed.run with two ranks over the shared-segment exchange (two processes time-slicing ONE GPU is
    not a configuration the product is meant for: this checks the launch path).  Round 3 saw one run in ~15 lose a rank after a
    20 s stall and repeated the run; the cause was bench.py's settling loop, in which every rank consulted ITS OWN clock to decide
    whether to run another block of 50 registrations - each of them a collective once an exchange is attached.  When the 0.5 s
    mark fell between two ranks' checks one rank ran a block the other never answered, and the exchange's bounded wait expired.
    The ranks now agree on the count; KICP_BENCH_RANK_SKEW_S starts their clocks 0.3 s apart here, which made the old loop fail
    every time.  No retry."""
    env = dict(os.environ, KICP_BENCH_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0", KICP_BENCH_RANK_SKEW_S="0.3")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full", "--steps", "3", "--warmup", "1", "--scans-per-step", "4",
           "--workload", "cfg1", "--comm", "shm", "--pg-backend", "gloo", "--no-cpu-baseline", "--no-sharded-cfg5"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    # (the first rank's own traceback first - the other rank only reports the closed connection)
    report = "\n".join([l for l in p.stderr.splitlines() if "[rank0]" in l][-40:]) + "\n...\n" + p.stderr[-6000:]
    assert p.returncode == 0, report
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["value"] > 0 and out["scaling"] == "strong"
    assert out["config"]["max_pose_abs_diff_vs_oracle"] < 1e-9
    assert out["roofline"]["kernel_avg_us"] > 0
    assert out["value_shm"] == out["value"] and out["value_p2p"] is not None and "value_rccl" in out  # every exchange at top level


def _p2p_worker(rank, world, barrier, handles, q):
    """peer-mailbox exchange (kicp_reg_p2p_*): `world` processes, one rank each.  With one GPU in the box all ranks sit on
    device 0 and reach each other's mailboxes through IPC mappings of the same HBM - the code path (export / open / stores
    into every mailbox / polling of the own one / rank-order sum) is the one GPUs of a node take over xGMI."""
    sys.path.insert(0, ROOT)
    try:
        import kinematic_icp_amd as K
        dev = rank % K.device_count()
        reg = K.KinematicRegistration(device=dev)
        handles[rank] = reg.p2p_export(world, rank)
        barrier.wait()
        reg.p2p_connect([handles[r] for r in range(world)])
        barrier.wait()
        out = _run_cases(reg, world, rank)  # default wire format: every first-level group's row goes to every rank
        # a second round on the same mailboxes (tags and buffer parity keep advancing), then the plain path after a detach
        out2 = _run_cases(reg, world, rank)
        # more sub-lanes per query = more workgroups = more group rows per rank; a rank that sends its total as one row (what a launch
        # beyond the mailbox's row limit does) pairs up with ranks that send group rows
        reg.set_option("small", 0), reg.set_option("lanes_per_query", 4)
        out3 = _run_cases(reg, world, rank)
        reg.set_option("lanes_per_query", 0)
        if rank == 0:
            reg.set_option("debug_p2p_one_row", 1)
        out4 = _run_cases(reg, world, rank)
        barrier.wait()
        reg.set_option("debug_p2p_one_row", 0)
        out5 = _run_cases(reg, world, rank)
        barrier.wait()
        reg.p2p_destroy()
        for other in (out2, out3, out4, out5):
            assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(out, other))
        q.put((rank, out, None))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, [], repr(e) + "\n" + traceback.format_exc()))
        try:
            barrier.abort()
        except Exception:  # noqa: BLE001
            pass


@pytest.mark.parametrize("world", [2, 3])
def test_peer_mailbox_exchange_across_processes(world):
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        handles = mgr.dict()
        results = _spawn(_p2p_worker, world, (ctx.Barrier(world), handles))
    ref = _single_process_results()
    for r in range(world):
        for (pose, iters), (pose1, iters1) in zip(results[r], ref):
            assert iters == iters1 and np.array_equal(pose, pose1)  # exact integer sums in rank order: the single-GPU bits


def test_peer_mailbox_reports_a_missing_peer():
    """A rank whose peers never write (here: a 2-rank mailbox with nobody on the other side) must come back with
    KICP_ERR_COMM after the in-kernel time-out instead of hanging."""
    import kinematic_icp_amd as K
    g = np.load(GOLD)
    reg = K.KinematicRegistration()
    h = reg.p2p_export(2, 0)
    reg2 = K.KinematicRegistration()          # the would-be peer: exports a mailbox but never registers anything
    try:
        h2 = reg2.p2p_export(2, 1)
        reg.p2p_connect([h, h2])
    except K.KicpError:
        pytest.skip("IPC handles cannot be opened inside the process that created them on this runtime")
    m = K.VoxelHashMap(float(g["a_voxel"]), float(g["a_maxrange"]), 20)
    m.AddPoints(g["a_map"])
    with pytest.raises(K.KicpError) as e:
        reg.ComputeRobotMotion(g["a_frame"], m, g["a_last"], g["a_rel"], float(g["a_tau"]))
    assert e.value.code == K.KICP_ERR_COMM
    reg.p2p_destroy(), reg2.p2p_destroy()
    reg.ComputeRobotMotion(g["a_frame"], m, g["a_last"], g["a_rel"], float(g["a_tau"]))  # usable again, single GPU


def _p2p_timeout_worker(rank, world, barrier, handles, q):
    """rank 0 registers, rank 1 connects its mailbox but never shows up: rank 0's kernel must give up after its bounded
    wait and the call must come back with KICP_ERR_COMM (then work again, single GPU)."""
    sys.path.insert(0, ROOT)
    os.environ["KICP_WAIT_TIMEOUT_S"] = "3"  # (the bound every wait inside the library shares; default 20 s - read once per process)
    try:
        import kinematic_icp_amd as K
        g = np.load(GOLD)
        reg = K.KinematicRegistration(device=0)
        handles[rank] = reg.p2p_export(world, rank)
        barrier.wait()
        reg.p2p_connect([handles[r] for r in range(world)])
        barrier.wait()
        out = None
        if rank == 0:
            m = K.VoxelHashMap(float(g["a_voxel"]), float(g["a_maxrange"]), 20)
            m.AddPoints(g["a_map"])
            try:
                reg.ComputeRobotMotion(g["a_frame"][:1000], m, g["a_last"], g["a_rel"], float(g["a_tau"]))
                out = "no error"
            except K.KicpError as e:
                out = e.code
        barrier.wait()
        reg.p2p_destroy()
        if rank == 0:
            pose = reg.ComputeRobotMotion(g["a_frame"], m, g["a_last"], g["a_rel"], float(g["a_tau"]))
            out = (out, bool(np.allclose(pose, g["a_pose"], rtol=0, atol=1e-9)))
        q.put((rank, out, None))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, None, repr(e) + "\n" + traceback.format_exc()))
        try:
            barrier.abort()
        except Exception:  # noqa: BLE001
            pass


def test_peer_mailbox_gives_up_on_a_silent_peer():
    import kinematic_icp_amd as K
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        results = _spawn(_p2p_timeout_worker, 2, (ctx.Barrier(2), mgr.dict()))
    assert results[0] == (K.KICP_ERR_COMM, True)
