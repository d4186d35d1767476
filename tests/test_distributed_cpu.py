"""The N>1 path on CPU: world_size-2 processes, the product's own TCP rendezvous, island
sharding and the evidence gather.  (The device-side gather is RCCL inside libsmc_hip; on the
GPU-less container the Group is created with device_collective=False, which exercises the same
sharding / ordering logic over the host star.)  torch.distributed/gloo appears here only as an
independent cross-check of the gathered values -- the product does not import torch."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

WORKER = r"""
import os, sys, json
sys.path.insert(0, {root!r})
sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import conftest                      # selects the emulator library when there is no GPU
conftest.pytest_configure(type("C", (), {{"addinivalue_line": lambda *a: None}})())
import particles_amd as pa
from particles_amd import kalman, state_space_models as ssm
from particles_amd.distributed import Group, shard_islands, log_mean_exp_host

grp = Group(device_collective=os.environ.get("SMC_TEST_RCCL") == "1")
TOTAL = 6
first, count = shard_islands(TOTAL, grp.rank, grp.world)
rng = np.random.RandomState(42)
x = np.cumsum(rng.standard_normal(12))
y = [np.array([v]) for v in x + 0.2 * rng.standard_normal(12)]
fk = ssm.Bootstrap(ssm=kalman.ToySSM(0.2), data=y)
pf = pa.SMC(fk=fk, N=1500, seed=77, n_islands=count, island_offset=first, collect="off")
pf.run()
grp.barrier()
if os.environ.get("SMC_TEST_MIGRATE") == "1":
    # a global theta-level resampling in the middle of the run: every rank applies the same
    # global source map, whole island states cross ranks, the run continues
    pf2 = pa.SMC(fk=fk, N=1500, seed=77, n_islands=count, island_offset=first, collect="off")
    pf2.step_async(5)
    src = np.array([4, 4, 0, 5, 1, 2])
    grp.migrate_islands(pf2, src)
    pf2.step_async(7)
    pf = pf2
allv = grp.gather_evidence(pf.logLts_islands)
tmax = grp.allreduce_max_host(float(grp.rank))
vmax = grp.allreduce_max_host(np.array([1.0 + grp.rank, 5.0 - grp.rank]))
gloo = None
if grp.world > 1 and os.environ.get("SMC_TEST_GLOO") == "1":
    import torch, torch.distributed as dist          # test-only cross-check
    os.environ["MASTER_PORT"] = os.environ["GLOO_PORT"]
    dist.init_process_group("gloo", rank=grp.rank, world_size=grp.world)
    outs = [torch.zeros(count, dtype=torch.float64) for _ in range(grp.world)]
    dist.all_gather(outs, torch.from_numpy(pf.logLts_islands.copy()))
    gloo = np.concatenate([o.numpy() for o in outs]).tolist()
    dist.destroy_process_group()
assert "torch" not in sys.modules or gloo is not None, "the product path imported torch"
if grp.rank == 0:
    print("RESULT " + json.dumps({{"ll": allv.tolist(), "tmax": tmax, "world": grp.world,
                                   "vmax": vmax.tolist(), "gloo": gloo,
                                   "path": grp.evidence_path,
                                   "lme": log_mean_exp_host(allv)}}))
grp.close()
"""


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fake_rccl_env(tmp_path):
    """Environment that makes the emulator build of smc_comm bind the RCCL test double."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    return {"SMC_RCCL_LIBRARY": build_emu.build_fake_rccl(), "SMC_TEST_RCCL": "1", "TMPDIR": str(tmp_path)}


def _run_world(world, tmp_path, gloo=False, migrate=False, **env_extra):
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT))
    port, gport = _free_port(), _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SMC_HIP_DEVICE="0",
                   GLOO_PORT=str(gport), SMC_TEST_GLOO="1" if gloo else "0",
                   SMC_TEST_MIGRATE="1" if migrate else "0", **env_extra)
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    import json
    line = [l for l in outs[0].splitlines() if l.startswith("RESULT ")][0]
    return json.loads(line[7:])


def test_rendezvous_messages_are_bound_to_direction_and_counter():
    """The host star's messages carry HMAC(secret, direction + round counter + payload): a recorded message is refused
    in another round (replay) and in the other direction (reflection); a length prefix beyond what the handshake
    expects is refused before anything is buffered; the handshake proves knowledge of the secret on both sides
    (challenge-response: the secret itself never crosses the socket) -- ADVICE r5."""
    import socket
    import struct
    from particles_amd import distributed as D
    a, b = socket.socketpair()
    key = b"secret-of-the-launch"
    seq0, seq1 = struct.pack("<Q", 0), struct.pack("<Q", 1)
    D._send_msg(a, b"payload", key, b"u" + seq0)
    assert D._recv_msg(b, key, b"u" + seq0) == b"payload"
    for ctx in (b"u" + seq1, b"d" + seq0):            # replayed into the next round; reflected back at the sender
        D._send_msg(a, b"payload", key, b"u" + seq0)
        with pytest.raises(ConnectionError, match="authentication"):
            D._recv_msg(b, key, ctx)
    a.sendall(struct.pack("<I", 1 << 30))             # "a hello of a gigabyte"
    with pytest.raises(ConnectionError, match="at most 64"):
        D._recv_msg(b, maxlen=64)
    assert D._mac(key, b"hello", b"1", b"c") != D._mac(key, b"ok", b"1", b"c")
    assert D._mac(key, b"hello", b"1", b"c") != D._mac(b"other", b"hello", b"1", b"c")
    a.close()
    b.close()


def test_shard_islands_partition():
    from particles_amd.distributed import shard_islands
    for total in (1, 5, 8, 256):
        for world in (1, 2, 3, 8):
            parts = [shard_islands(total, r, world) for r in range(world)]
            assert sum(c for _, c in parts) == total
            assert parts[0][0] == 0
            for (f0, c0), (f1, _) in zip(parts, parts[1:]):
                assert f0 + c0 == f1


def test_world2_matches_world1(tmp_path, has_gpu):
    """Sharding 6 islands over 2 ranks gives exactly the single-process answer,
    in global island order (results do not depend on the number of GPUs)."""
    one = _run_world(1, tmp_path)
    two = _run_world(2, tmp_path, gloo=True)
    three = _run_world(3, tmp_path)
    assert two["world"] == 2 and two["tmax"] == 1.0 and two["vmax"] == [2.0, 5.0]
    assert two["gloo"] == two["ll"]                 # the star's gather == gloo's all_gather
    assert two["path"].startswith("host-fallback") and one["path"] == "none"
    assert three["world"] == 3 and three["ll"] == one["ll"] and three["vmax"] == [3.0, 5.0]
    assert len(one["ll"]) == 6 and one["ll"] == two["ll"]
    assert one["lme"] == two["lme"]
    assert len(set(one["ll"])) == 6


def test_island_migration_world2_and_3_match_world1(tmp_path):
    """migrate_islands: a global permutation of whole filters across ranks (packed island states
    through one all-to-all) gives the single-process permute_islands result bit for bit -- and
    the run continues identically afterwards (Philox streams tied to the global slot)."""
    one = _run_world(1, tmp_path, migrate=True)
    two = _run_world(2, tmp_path, migrate=True)
    three = _run_world(3, tmp_path, migrate=True)
    assert one["ll"] == two["ll"] == three["ll"]
    assert one["ll"][0] == one["ll"][1] or abs(one["ll"][0] - one["ll"][1]) < 50    # (copies evolve apart)
    import numpy as np
    base = _run_world(1, tmp_path)
    assert not np.allclose(base["ll"], one["ll"])          # the permutation did change the run


SMC2_WORKER = r"""
import os, sys, json
sys.path.insert(0, {root!r})
sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import conftest
conftest.pytest_configure(type("C", (), {{"addinivalue_line": lambda *a: None}})())
from particles_amd import kalman, smc2
from particles_amd.distributed import Group

grp = Group(device_collective=os.environ.get("SMC_TEST_RCCL") == "1")
rng = np.random.RandomState(4)
T = int(os.environ.get("SMC_TEST_T", "14"))
x = np.cumsum(rng.standard_normal(T))
y = [np.array([v]) for v in x + 0.3 * rng.standard_normal(T)]
prior = smc2.IndepPrior(sigmaY=("lognormal", np.log(0.8), 1.2))
kw = dict(ssm_cls=lambda sigmaY: kalman.LinearGauss(rho=1.0, sigmaX=1.0, sigmaY=sigmaY, sigma0=1.0),
          prior=prior, data=y, init_Nx=int(os.environ.get("SMC_TEST_NX", "128")), N=12, seed=5,
          ESSrmin=0.8, nmcmc=2, ar_to_increase_Nx=float(os.environ.get("SMC_TEST_AR", "-1")), max_Nx=256)
if os.environ.get("SMC_TEST_WF") == "1":       # waste-free move: 6 chains x 2 states = the same 12 theta-particles
    kw.update(N=6, wastefree=True, len_chain=2)
alg = smc2.ShardedSMC2(group=grp, **kw)
alg.run()
single = None
if grp.world == 1:                 # the one-GPU class (theta level on the device) on the same problem
    ref = smc2.SMC2(**kw)
    ref.run()
    single = {{"lw": ref.lw.tolist(), "theta": ref.theta["sigmaY"].tolist(), "logLt": ref.logLt,
               "moves": len(ref.move_times), "ESSs": ref.ESSs, "logLts": ref.logLts, "Nx": ref.Nx}}
if grp.rank == 0:
    print("RESULT " + json.dumps({{"lw": alg.lw.tolist(), "theta": alg.theta["sigmaY"].tolist(),
                                   "logLt": alg.logLt, "ESSs": alg.ESSs, "moves": len(alg.move_times),
                                   "acc": alg.acc_rates, "Nx": alg.Nx, "path": grp.evidence_path,
                                   "device_theta": alg.device_theta, "logLts": alg.logLts,
                                   "local": alg.pf.n_islands, "single": single}}))
grp.close()
"""


def _run_smc2_world(world, tmp_path, **env_extra):
    script = tmp_path / "smc2_worker.py"
    script.write_text(SMC2_WORKER.format(root=ROOT))
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SMC_HIP_DEVICE="0", **env_extra)
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=900)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    import json
    line = [l for l in outs[0].splitlines() if l.startswith("RESULT ")][0]
    return json.loads(line[7:])


def test_sharded_smc2_is_world_invariant(tmp_path):
    """SMC^2 with the theta-population sharded over ranks (per-step all-gather of the evidence
    increments, theta-resampling = migration of whole filters, PMCMC moves local): the run is the
    same run for 1, 2 and 3 ranks -- theta-particles, theta-weights, evidence, ESS trajectory bit for
    bit -- and agrees with the one-GPU class whose theta level lives on the device."""
    one = _run_smc2_world(1, tmp_path)
    two = _run_smc2_world(2, tmp_path)
    three = _run_smc2_world(3, tmp_path)
    assert one["moves"] >= 1 and one["local"] == 12 and two["local"] == 6 and three["local"] == 4
    for other in (two, three):
        for k in ("lw", "theta", "logLt", "ESSs", "moves", "acc", "Nx"):
            assert one[k] == other[k], k
    assert np.isfinite(one["logLt"]) and len(one["ESSs"]) == 14
    # the one-GPU class accumulates the theta-weights on the device (increment by increment), this one
    # differences the cumulated evidences: ulps apart, same decisions
    s = one["single"]
    assert s["moves"] == one["moves"] and np.allclose(s["theta"], one["theta"], rtol=1e-12, atol=0)
    assert np.allclose(s["lw"], one["lw"], rtol=0, atol=1e-9) and abs(s["logLt"] - one["logLt"]) < 1e-9
    # with the exchange step (N_x doubles when moves are rejected too often)
    e1 = _run_smc2_world(1, tmp_path, SMC_TEST_AR="1.01", SMC_TEST_T="8")
    e2 = _run_smc2_world(2, tmp_path, SMC_TEST_AR="1.01", SMC_TEST_T="8")
    assert e1["Nx"] == 256 and all(e1[k] == e2[k] for k in ("lw", "theta", "logLt", "ESSs", "Nx"))


def test_sharded_wastefree_smc2_is_world_invariant(tmp_path):
    """The waste-free move (MCMCSequenceWF, smc_samplers.py:669-684: every state of every chain kept with its filter) on a
    population sharded over ranks: the chains' starting filters cross ranks (Group.move_islands), each rank
    runs its share of the chains, the new population is assembled across ranks -- worlds 2 and 3 are the same run as world 1
    bit for bit, over the host star and through the RCCL double, and world 1 agrees with the one-process class."""
    one = _run_smc2_world(1, tmp_path, SMC_TEST_WF="1")
    assert one["moves"] >= 1 and one["local"] == 12
    for world in (2, 3):
        other = _run_smc2_world(world, tmp_path, SMC_TEST_WF="1")
        assert other["local"] == 12 // world
        for k in ("lw", "theta", "logLt", "ESSs", "moves", "acc", "Nx"):
            assert one[k] == other[k], (world, k)
    s = one["single"]
    assert s["moves"] == one["moves"] and np.allclose(s["theta"], one["theta"], rtol=1e-12, atol=0)
    assert np.allclose(s["lw"], one["lw"], rtol=0, atol=1e-9) and abs(s["logLt"] - one["logLt"]) < 1e-9
    two_rccl = _run_smc2_world(2, tmp_path, SMC_TEST_WF="1", **_fake_rccl_env(tmp_path))
    assert two_rccl["path"] == "rccl" and two_rccl["device_theta"]
    # (the device theta level accumulates the weights increment by increment, the host form differences cumulated
    #  evidences: the proposal covariance, hence theta, agrees to rounding; same decisions)
    assert one["moves"] == two_rccl["moves"] and one["Nx"] == two_rccl["Nx"]
    assert np.allclose(one["theta"], two_rccl["theta"], rtol=1e-12, atol=0)
    assert np.allclose(one["lw"], two_rccl["lw"], rtol=0, atol=1e-9) and abs(one["logLt"] - two_rccl["logLt"]) < 1e-9


def test_multi_rank_rccl_calls_through_the_test_double(tmp_path, has_gpu):
    """The device-collective branch of the Group with 2 and 3 ranks -- ncclCommInitRank, ncclAllGather,
    grouped ncclSend / ncclRecv -- against tests/emu/fake_rccl.c, which moves the bytes between the
    emulator processes and refuses protocol violations (datatype codes, counts that differ between a
    matched pair, point-to-point calls outside a group): evidences, island migration and the sharded
    SMC^2 give what the host star and the single process give, and `evidence_path` says "rccl"."""
    if has_gpu:
        pytest.skip("the test double stands in for RCCL on GPU-less boxes")
    env = _fake_rccl_env(tmp_path)
    one = _run_world(1, tmp_path)
    for world in (2, 3):
        got = _run_world(world, tmp_path, **env)
        assert got["path"] == "rccl" and got["world"] == world and got["ll"] == one["ll"]
    m1 = _run_world(1, tmp_path, migrate=True)
    m3 = _run_world(3, tmp_path, migrate=True, **env)
    assert m3["path"] == "rccl" and m3["ll"] == m1["ll"]
    # sharded SMC^2 with its theta level ON THE DEVICE (smc_filter_theta_enable_sharded: ncclAllGather of the
    # increments enqueued behind every step, `sync_every` steps per host synchronisation): worlds 1, 2, 3
    # are the same run, and so is the one-GPU class -- bit for bit, the same kernel on the same N values
    s1 = _run_smc2_world(1, tmp_path, **env)
    s2 = _run_smc2_world(2, tmp_path, **env)
    s3 = _run_smc2_world(3, tmp_path, **env)
    assert s2["path"] == "rccl" and s1["device_theta"] and s2["device_theta"] and s3["device_theta"]
    assert s1["moves"] >= 1 and s2["local"] == 6 and s3["local"] == 4
    for k in ("lw", "theta", "logLt", "ESSs", "logLts", "moves", "acc", "Nx"):
        assert s1[k] == s2[k] == s3[k], k
    single = s1["single"]
    for k in ("lw", "theta", "logLt", "ESSs", "logLts", "moves", "Nx"):
        assert single[k] == s1[k], k
    # ... with the exchange step (a new batch adopts the replicated theta-weights)
    e1 = _run_smc2_world(1, tmp_path, SMC_TEST_AR="1.01", SMC_TEST_T="8", **env)
    e2 = _run_smc2_world(2, tmp_path, SMC_TEST_AR="1.01", SMC_TEST_T="8", **env)
    assert e1["Nx"] == 256 and all(e1[k] == e2[k] for k in ("lw", "theta", "logLt", "ESSs", "Nx"))
    assert all(e1["single"][k] == e1[k] for k in ("lw", "theta", "logLt", "ESSs", "Nx"))
    # the per-step host form (no device collective) decides the same and agrees to rounding
    h2 = _run_smc2_world(2, tmp_path)
    assert not h2["device_theta"] and h2["moves"] == s2["moves"] and h2["theta"] == s2["theta"]
    assert np.allclose(h2["lw"], s2["lw"], rtol=0, atol=1e-9)


MULTI_WORKER = r"""
import os, sys, json
sys.path.insert(0, {root!r})
sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import conftest
conftest.pytest_configure(type("C", (), {{"addinivalue_line": lambda *a: None}})())
import particles_amd as pa
from particles_amd import kalman, state_space_models as ssm
from particles_amd.distributed import Group

grp = Group(device_collective=os.environ.get("SMC_TEST_RCCL") == "1")
rng = np.random.RandomState(42)
x = np.cumsum(rng.standard_normal(10))
y = [np.array([v]) for v in x + 0.2 * rng.standard_normal(10)]
fk = ssm.Bootstrap(ssm=kalman.ToySSM(0.2), data=y)
np.random.seed(5 + grp.rank)          # the ranks' numpy streams differ: rank 0's seeds must win
# (1) the C5 shape: nruns islands, a float per run -> the RCCL all-gather
r1 = pa.multiSMC(nruns=7, fk=fk, N=[600, 1100], resampling="systematic", group=grp,
                 out_func=lambda pf: pf.logLt)
# (2) an array per run (the evidence trajectory)
r2 = pa.multiSMC(nruns=5, fk=fk, N=600, group=grp, out_func=lambda pf: np.array(pf.logLts))
# (3) objects: pickled over the star
r3 = pa.multiSMC(nruns=4, fk=fk, N=600, group=grp, out_func=lambda pf: {{"ll": pf.logLt, "N": pf.N}})
# (4) no out_func: the unbatched path, a host snapshot of every run; fewer runs than ranks at world 3
r4 = pa.multiSMC(nruns=2, fk=fk, N=400, group=grp)
if grp.rank == 0:
    print("RESULT " + json.dumps({{
        "r1": [[d["run"], d["seed"], d["N"], d["output"]] for d in r1],
        "r2": [[d["run"], d["seed"], d["output"].tolist()] for d in r2],
        "r3": [[d["run"], d["seed"], d["output"]] for d in r3],
        "r4": [[d["run"], d["seed"], d["output"].logLt, float(d["output"].X.sum()), d["output"].t] for d in r4],
        "types": [type(r1[0]["output"]).__name__, type(r2[0]["output"]).__name__, type(r4[0]["output"]).__name__],
        "path": grp.evidence_path}}))
grp.close()
"""


def _run_multi_world(world, tmp_path, **env_extra):
    import json
    script = tmp_path / "multi_worker.py"
    script.write_text(MULTI_WORKER.format(root=ROOT))
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SMC_HIP_DEVICE="0", **env_extra)
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=900)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    return json.loads([l for l in outs[0].splitlines() if l.startswith("RESULT ")][0][7:])


def test_multiSMC_over_a_group_is_world_invariant(tmp_path, has_gpu):
    """The reference's multi-run seam (core.py:431-518, utils.py:158-186) over one process per GPU:
    `multiSMC(..., group=Group())` called by every rank shards the runs, gathers the outputs in run
    order and returns the reference's list of dicts -- worlds 2 and 3 (host star, and the RCCL
    branch through the protocol-checking double) equal the world-1 result bit for bit."""
    one = _run_multi_world(1, tmp_path)
    assert one["types"] == ["float", "ndarray", "SMC"]          # one process: the SMC objects themselves
    assert [r[0] for r in one["r1"]] == list(range(7)) * 2 and [r[2] for r in one["r1"]] == [600] * 7 + [1100] * 7
    assert len({r[3] for r in one["r1"]}) == 14                     # distinct streams per run and per N
    assert len(one["r2"]) == 5 and len(one["r2"][0][2]) == 10 and len(one["r4"]) == 2 and one["r4"][0][4] == 10
    for world in (2, 3):
        got = _run_multi_world(world, tmp_path)
        assert got["path"].startswith("host-fallback")
        for k in ("r1", "r2", "r3", "r4"):
            assert got[k] == one[k], (world, k)
        assert got["types"][:2] == ["float", "ndarray"] and got["types"][2] == "RunSnapshot"
    if not has_gpu:
        env = _fake_rccl_env(tmp_path)
        for world in (2, 3):
            got = _run_multi_world(world, tmp_path, **env)
            assert got["path"] == "rccl"
            for k in ("r1", "r2", "r3", "r4"):
                assert got[k] == one[k], (world, k)


def test_rccl_test_double_refuses_protocol_violations(tmp_path):
    """The double itself: what it accepts is what RCCL accepts from smc_comm, what it refuses would
    deadlock or corrupt on a node."""
    import ctypes
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    L = ctypes.CDLL(build_emu.build_fake_rccl())
    L.ncclGetErrorString.restype = ctypes.c_char_p

    class Uid(ctypes.Structure):
        _fields_ = [("internal", ctypes.c_char * 128)]
    os.environ["TMPDIR"] = str(tmp_path)
    uid = Uid()
    assert L.ncclGetUniqueId(ctypes.byref(uid)) == 0
    comm = ctypes.c_void_p()
    assert L.ncclCommInitRank(ctypes.byref(comm), 1, uid, 0) == 0
    a = (ctypes.c_double * 4)(1, 2, 3, 4)
    b = (ctypes.c_double * 4)()
    assert L.ncclAllGather(a, b, ctypes.c_size_t(4), 8, comm, None) == 0 and list(b) == [1, 2, 3, 4]
    assert L.ncclAllGather(a, b, ctypes.c_size_t(4), 7, comm, None) != 0                       # ncclFloat is not ours
    assert b"datatype" in L.ncclGetErrorString(4)
    assert L.ncclSend(a, ctypes.c_size_t(32), 0, 0, comm, None) != 0                            # outside a group
    assert b"outside ncclGroupStart" in L.ncclGetErrorString(5)
    assert L.ncclGroupStart() == 0
    assert L.ncclSend(a, ctypes.c_size_t(32), 0, 0, comm, None) == 0
    assert L.ncclRecv(b, ctypes.c_size_t(16), 0, 0, comm, None) == 0                            # 16 != 32 bytes
    assert L.ncclGroupEnd() != 0 and b"byte count differs" in L.ncclGetErrorString(5)
    assert L.ncclGroupStart() == 0
    assert L.ncclSend(a, ctypes.c_size_t(32), 0, 3, comm, None) != 0                            # peer out of range
    assert L.ncclGroupEnd() == 0
    assert L.ncclGroupEnd() != 0                                                                # unbalanced
    bad = Uid()
    assert L.ncclCommInitRank(ctypes.byref(ctypes.c_void_p()), 2, bad, 0) != 0                  # an id nobody made
    assert L.ncclCommDestroy(comm) == 0


def test_bench_two_ranks_launch_line(tmp_path):
    """The driver's N = 2 launch line of bench.py, through the emulator (both ranks on 'device' 0):
    the N > 1 path -- rendezvous, island offsets per rank, max-over-ranks timing, the separately timed
    evidence gather, the labelled host fallback -- must produce the one JSON line with its contract keys."""
    import json
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    env = dict(os.environ, SMC_TEST_EMULATOR="1", SMC_HIP_LIBRARY=build_emu.build(), SMC_BENCH_NGPU="1",
               MASTER_ADDR="127.0.0.1")
    env.pop("SMC_ALLOW_HOST_GATHER", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "3", "--warmup", "1", "--log2N", "11", "--reps", "2",
           "--no-cpu-baseline", "--no-profile", "--full"]
    # without RCCL the launch line FAILS, and says why in a JSON object (a scale line is never a host-star line
    # by accident) ...
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert p.returncode != 0
    err = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(err) == 1 and "RCCL" in err[0]["error"] and err[0]["rccl"] is False and "value" not in err[0]
    # ... unless the caller opts into the labelled host gather
    cmd[cmd.index("--master-port") + 1] = str(_free_port())
    p = subprocess.run(cmd + ["--allow-host-gather"], env=env, capture_output=True, text=True, timeout=600,
                       cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                   # rank 0 prints ONE line
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == "weak" and d["value"] > 0
    assert d["rccl"] is False and d["evidence_gather"].startswith("host-fallback")
    assert len(d["logLt"]) == 2 and d["logLt"][0] != d["logLt"][1]      # one filter per rank, distinct streams
    assert d["evidence_gather_ms"] is not None and "timing" in d and "note" in d["timing"]
    assert d["timing"]["ms_per_step_with_gather"] >= d["ms_per_step"] * 0.5      # the region that holds the collective
    assert "RCCL unavailable" in p.stderr
    # C5 under the same launch line is ONE call of the reference's multiSMC per rank (bench.py's `multiSMC` block)
    cmd5 = list(cmd)
    cmd5[cmd5.index("--master-port") + 1] = str(_free_port())
    cmd5[cmd5.index("--log2N") + 1] = "10"
    p = subprocess.run(cmd5 + ["--allow-host-gather", "--workload", "c5", "--islands", "3"], env=env,
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    d5 = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    m = d5["multiSMC"]
    assert m["nruns"] == 6 and m["distinct_runs"] == 6 and m["value"] > 0 and "multiSMC(nruns=6" in m["call"]
    assert m["evidence_gather"].startswith("host-fallback") and d5["config"]["islands_per_gpu"] == 3


def test_bench_eight_rank_c5_line_through_the_rccl_double(tmp_path, has_gpu):
    """BASELINE config C5 as the driver launches it on an 8-GPU node -- `bench.py --gpus 8 --workload c5`: 8 ranks, one
    device each, 32 islands per rank, the log-evidences gathered by the library's RCCL all-gather -- on the emulator
    (8 pretended devices) with tests/emu/fake_rccl.c standing in for RCCL: the line says rccl: true, names 8 distinct
    devices, and its multiSMC block holds 256 distinct runs (the 8-GPU line is ready, unmeasured)."""
    import json
    if has_gpu:
        pytest.skip("the test double stands in for RCCL on GPU-less boxes")
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    env = dict(os.environ, SMC_TEST_EMULATOR="1", SMC_HIP_LIBRARY=build_emu.build(), SMC_EMU_NDEV="8", **_fake_rccl_env(tmp_path))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "SMC_ALLOW_HOST_GATHER", "SMC_BENCH_NGPU"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--workload", "c5", "--log2N", "10", "--steps", "2",
           "--warmup", "1", "--reps", "1", "--no-cpu-baseline", "--no-profile", "--full"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1200, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["rccl"] is True and d["evidence_gather"] == "rccl" and d["scaling"] == "weak"
    assert len(d["rank_devices"]) == 8 and len(set(d["rank_devices"])) == 8
    assert d["config"]["islands_per_gpu"] == 32 and d["value"] > 0
    m = d["multiSMC"]
    assert m["nruns"] == 256 and m["distinct_runs"] == 256 and m["evidence_gather"] == "rccl" and np.isfinite(m["log_mean_exp_evidence"])


def test_bench_spawns_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` WITHOUT a launcher (no RANK / WORLD_SIZE in the environment): bench.py spawns its two
    ranks itself over the library's TCP rendezvous -- the scale line does not depend on torch.distributed.run (VERDICT r4,
    item 9) -- and rank 0 prints the one JSON line."""
    import json
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    env = dict(os.environ, SMC_TEST_EMULATOR="1", SMC_HIP_LIBRARY=build_emu.build(), SMC_BENCH_NGPU="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "SMC_ALLOW_HOST_GATHER"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--log2N", "11",
           "--reps", "2", "--no-cpu-baseline", "--no-profile", "--allow-host-gather"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and len(d["logLt"]) == 2 and d["logLt"][0] != d["logLt"][1]
