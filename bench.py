#!/usr/bin/env python3
"""Headline benchmark: train imgs/sec of the IR-50-layout ResNet50 + ArcFace/PartialFC head on synthetic 112x112
faces (BASELINE.json metric), one process per GPU.

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W
  python bench.py --gpus N ...            (no launcher: starts the N ranks itself, as a child torch.distributed.run)

A step = Model.training_step (zero_grad, backbone fwd, normalise, margin-softmax head, backward, clip, SGD step)
on a pre-staged synthetic batch.  Rank 0 prints ONE JSON line.  `--dump-outputs DIR` also writes what the last timed step
produced (its loss and the model state it left, larger tensors as a fixed seeded sample) to DIR/<name>.npy, so that two builds
can be compared output for output on identical seeded inputs.  `roofline` is measured live: every launch of the
dominant kernel (the bf16 MFMA implicit-GEMM conv, forward + data-gradient) inside the timed region is bracketed
by HIP events on the stream it runs on; achieved = algorithmic FLOPs of those launches / their summed duration.
`cpu_baseline` times the CPU restatement (oracle/) of the same step on the host cores (rank 0, N=1 only).
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "face-recognition-pytorch_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

BF16_DENSE_PEAK_TFLOPS = 2516.6      # 256 CU x 4096 FLOP/clk x 2.4 GHz (MI355X_MICROARCH.md: ~2.5 PF dense)
NUM_CLASSES = 122000                 # BASELINE.json cfg 2 ("MS1M-122K ids"); the reference config has 86 690
BATCH = 512


def make_conf(args, rank, world):
    rate = 1.0 if world == 1 else 0.1            # cfg 2 (1 GPU, full head) / cfg 3 (PartialFC rate 0.1 over the node)
    return types.SimpleNamespace(
        network=args.network, emd_size=512, img_size=args.img_size, local_rank=rank % max(torch.cuda.device_count(), 1),
        world_size=world, sample_rate=rate, mixed_precision=True, loss_s=30.0, loss_m=0.35, n_classes=args.classes,
        optimizer="SGD", lr=0.1, wd=5e-4, mom=0.9, loss="PartialFC", lr_scheduler=None, frhip_dtype="bf16",
        ckpt_path=None)


class ConvMeter:
    """Roofline probe for the dominant kernel (the bf16 MFMA implicit-GEMM conv: every forward and data-gradient
    convolution of the step).  `collect` records the arguments of every such launch during one eager step;
    `measure` re-issues exactly those launches back to back on the current stream between two HIP events, so the
    summed device time of the kernel is measured without host gaps (each launch runs >= 100 us, the host needs
    ~20 us to enqueue the next one)."""

    def __init__(self, ops):
        self.ops, self.calls, self.collect = ops, [], False
        self._fwd, self._dgrad = ops.conv_fwd, ops.conv_dgrad

        def conv_fwd(x, w, stride, pad, want_stats=True):
            if self.collect and x.dtype == torch.bfloat16:
                n, h, wd, c = x.shape
                k, r, s, _ = w.shape
                ho, wo = ops.conv_out_hw(h, wd, r, s, stride, pad)
                self.calls.append((self._fwd, (x, w, stride, pad, want_stats), 2.0 * n * ho * wo * k * r * s * c))
            return self._fwd(x, w, stride, pad, want_stats)

        def conv_dgrad(dy, wt, x_shape, r, s, stride, pad, residual=None, out=None, bnred=None, residual_stride=1):
            if self.collect and dy.dtype == torch.bfloat16:
                n, ho, wo, k = dy.shape
                # the probe re-issues the launch as the step does (incl. the fused BN-backward reduction in its epilogue)
                self.calls.append((self._dgrad, (dy, wt, tuple(x_shape), r, s, stride, pad, residual, None, bnred, residual_stride),
                                   2.0 * n * ho * wo * k * r * s * x_shape[3]))    # algorithmic MACs = forward's
            return self._dgrad(dy, wt, x_shape, r, s, stride, pad, residual, out, bnred, residual_stride)

        self._fwdx = ops.conv_fwd_bnrelu

        def conv_fwd_bnrelu(x, st, w, stride, pad, want_stats=True, act_out=None):
            if self.collect and x.dtype == torch.bfloat16:
                n, h, wd, c = x.shape
                k, r, s, _ = w.shape
                ho, wo = ops.conv_out_hw(h, wd, r, s, stride, pad)
                self.calls.append((self._fwdx, (x, st, w, stride, pad, want_stats, act_out), 2.0 * n * ho * wo * k * r * s * c))
            return self._fwdx(x, st, w, stride, pad, want_stats, act_out)

        ops.conv_fwd, ops.conv_dgrad, ops.conv_fwd_bnrelu = conv_fwd, conv_dgrad, conv_fwd_bnrelu

    def measure(self, repeats=3):
        torch.cuda.synchronize()
        for fn, a, _ in self.calls:            # untimed pass (page in code objects / L2)
            fn(*a)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(repeats):
            for fn, a, _ in self.calls:
                fn(*a)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / repeats
        fl = sum(f for _, _, f in self.calls)
        return len(self.calls), ms, fl

    # ---- in-step measurement: every conv launch of the TIMED steps bracketed by two HIP events on the stream it runs on
    def start_instep(self):
        self.instep, self._pool, self.collect = [], [], False
        ops, fwd, dgrad = self.ops, self._fwd, self._dgrad

        def ev():
            return self._pool.pop() if self._pool else torch.cuda.Event(enable_timing=True)

        def conv_fwd(x, w, stride, pad, want_stats=True):
            if x.dtype != torch.bfloat16:
                return fwd(x, w, stride, pad, want_stats)
            n, h, wd, c = x.shape
            k, r, s, _ = w.shape
            ho, wo = ops.conv_out_hw(h, wd, r, s, stride, pad)
            a, b = ev(), ev()
            a.record()
            out = fwd(x, w, stride, pad, want_stats)
            b.record()
            self.instep.append((a, b, 2.0 * n * ho * wo * k * r * s * c))
            return out

        def conv_dgrad(dy, wt, x_shape, r, s, stride, pad, residual=None, out=None, bnred=None, residual_stride=1):
            if dy.dtype != torch.bfloat16:
                return dgrad(dy, wt, x_shape, r, s, stride, pad, residual, out, bnred, residual_stride)
            n, ho, wo, k = dy.shape
            a, b = ev(), ev()
            a.record()
            res = dgrad(dy, wt, x_shape, r, s, stride, pad, residual, out, bnred, residual_stride)
            b.record()
            self.instep.append((a, b, 2.0 * n * ho * wo * k * r * s * x_shape[3]))
            return res

        fwdx = self._fwdx

        def conv_fwd_bnrelu(x, st, w, stride, pad, want_stats=True, act_out=None):
            n, h, wd, c = x.shape
            k, r, s, _ = w.shape
            ho, wo = ops.conv_out_hw(h, wd, r, s, stride, pad)
            a, b = ev(), ev()
            a.record()
            out = fwdx(x, st, w, stride, pad, want_stats, act_out)
            b.record()
            self.instep.append((a, b, 2.0 * n * ho * wo * k * r * s * c))
            self.instep_xf = getattr(self, "instep_xf", 0) + 1
            return out

        ops.conv_fwd_bnrelu = conv_fwd_bnrelu
        f8 = ops.conv_fwd_fp8
        self._f8, self.instep8 = f8, []

        def conv_fwd_fp8(x8, w8, wscale, stride, pad, want_stats=True):
            n, h, wd, c = x8.shape
            k, r, s, _ = w8.shape
            ho, wo = ops.conv_out_hw(h, wd, r, s, stride, pad)
            a, b = ev(), ev()
            a.record()
            out = f8(x8, w8, wscale, stride, pad, want_stats)
            b.record()
            self.instep8.append((a, b, 2.0 * n * ho * wo * k * r * s * c))
            return out

        ops.conv_fwd, ops.conv_dgrad, ops.conv_fwd_fp8 = conv_fwd, conv_dgrad, conv_fwd_fp8

    def stop_instep8(self):
        """fp8 forward convolutions recorded since start_instep(): (launches, summed kernel ms, algorithmic FLOP)"""
        ms = sum(a.elapsed_time(b) for a, b, _ in self.instep8)
        return len(self.instep8), ms, sum(f for _, _, f in self.instep8)

    def stop_instep(self):
        """-> (launches, summed kernel ms, algorithmic FLOP) over everything recorded since start_instep()"""
        self.ops.conv_fwd, self.ops.conv_dgrad, self.ops.conv_fwd_fp8, self.ops.conv_fwd_bnrelu = self._fwd, self._dgrad, self._f8, self._fwdx
        torch.cuda.synchronize()
        ms = sum(a.elapsed_time(b) for a, b, _ in self.instep)
        return len(self.instep), ms, sum(f for _, _, f in self.instep)


def csrc_digest():
    """content hash of the kernel sources: ties a committed PMC measurement to the kernels it was taken on"""
    import hashlib
    h = hashlib.sha1()
    d = os.path.join(PKG, "frhip", "csrc")
    for f in sorted(os.listdir(d)):
        if f.startswith(("igemm_halo", "igemm_nt", "common")):       # the forward / data-gradient conv kernels and what they include
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def pmc_traffic(args):
    """HBM bytes per launch of the dominant kernels from the committed rocprofv3 --pmc passes (FETCH_SIZE / WRITE_SIZE in
    separate runs, tools/pmc_run.sh) -- reported only when that measurement was taken on the kernels of THIS tree."""
    if args.network != "ResNet50" or args.batch != BATCH:
        return None, None
    best = None
    pdir = os.path.join(ROOT, "profiles")
    for f in sorted(os.listdir(pdir)) if os.path.isdir(pdir) else []:
        if f.endswith("_pmc_traffic.json"):
            rec = json.load(open(os.path.join(pdir, f)))
            if rec.get("csrc_digest") == csrc_digest():
                best = (rec.get("hbm_bytes_per_launch"), "profiles/" + f)
    return best if best is not None else (None, "no committed PMC pass matches the conv kernels of this tree")


def host_cores():
    """cores this process may really use: affinity mask capped by the cgroup CPU quota (the GPU box shows 256
    logical CPUs but grants a 16-CPU share; oversubscribing torch's pool makes the CPU leg crawl)."""
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            cores = min(cores, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, cores)


def cpu_baseline(classes, batch=16, steps=12):
    """Oracle (CPU restatement, fp32, all host cores) on a bounded sample of the same workload."""
    from oracle import recipe, resnet_ref, train_ref
    cores = host_cores()
    torch.set_num_threads(cores)
    log("cpu_baseline: %d threads" % cores)
    blocks = resnet_ref.BLOCKS["ResNet50"]
    sd = recipe.fill_state(resnet_ref.resnet_spec(blocks), 1)
    w = recipe.normal(2, (classes, 512), 0.01)
    img, ids = recipe.images(3, batch), recipe.labels(4, batch, classes)
    opt = train_ref.SGDState(0.1, 0.9, 5e-4)
    train_ref.train_step(sd, w, img, ids, blocks, classes, opt)       # warm-up
    log("cpu_baseline: warm-up step done")
    t0 = time.time()
    for i in range(steps):
        train_ref.train_step(sd, w, img, ids, blocks, classes, opt)
        log("cpu_baseline: step %d" % i)
    dt = time.time() - t0
    return {"value": round(batch * steps / dt, 2), "unit": "imgs/sec", "cores": cores, "kind": "port",
            "sample": "oracle/ CPU restatement, ResNet50 + ArcFace head C=%d, B=%d fp32, 1 warm-up + %d timed SGD "
                      "steps (%.1f s)" % (classes, batch, steps, dt)}


def cpu_baseline_cfg1(batch=16, steps=10):
    """BASELINE cfg 1 (the reference's own CPU-runnable case): ResNet-18 + ArcFace head, 256 ids, B = 16, fp32, all host cores"""
    from oracle import recipe, resnet_ref, train_ref
    cores = host_cores()
    torch.set_num_threads(cores)
    blocks = resnet_ref.BLOCKS["ResNet18"]
    sd = recipe.fill_state(resnet_ref.resnet_spec(blocks), 1)
    w = recipe.normal(2, (256, 512), 0.01)
    img, ids = recipe.images(3, batch), recipe.labels(4, batch, 256)
    opt = train_ref.SGDState(0.1, 0.9, 5e-4)
    for _ in range(3):
        train_ref.train_step(sd, w, img, ids, blocks, 256, opt)
    t0 = time.time()
    for _ in range(steps):
        train_ref.train_step(sd, w, img, ids, blocks, 256, opt)
    dt = time.time() - t0
    log("cpu_baseline_cfg1: %.2f s" % dt)
    return {"value": round(batch * steps / dt, 2), "unit": "imgs/sec", "cores": cores, "kind": "port",
            "sample": "oracle/ CPU restatement, BASELINE cfg 1: ResNet-18 + ArcFace head C=256, B=%d fp32, 3 warm-up + %d timed SGD steps (%.1f s)"
                      % (batch, steps, dt)}


FLOP_IMG = {"ResNet50": 33.92e9, "ResNet18": 10.3e9, "Swin34": 10.2e9,
            "AlterNet50": 6 * 2.1025e9}       # tools/count_macs.py: 2.1025 GMAC forward at 192 x 192


def extra_config(network, batch, fp8, classes, steps=10, warmup=3):
    """One more BASELINE configuration timed in this process after the headline line: same step loop,
    same barrier + synchronize bracket, K = `steps` after `warmup` untimed steps.  Returns the fields of a bench line."""
    from model.FR_PartialFC import Model
    a = types.SimpleNamespace(network=network, img_size=192 if network.startswith("AlterNet") else 112, classes=classes)
    conf = make_conf(a, 0, 1)
    conf.frhip_fp8 = bool(fp8)
    torch.manual_seed(1234)
    model = Model(conf, None, "train")
    model.sync_loss = False
    gen = torch.Generator().manual_seed(1234)
    img = torch.randn((batch, 3, a.img_size, a.img_size), generator=gen).clamp_(-1, 1).cuda()
    ids = torch.randint(0, classes, (batch,), generator=gen).cuda()
    for _ in range(warmup):
        model.training_step((img, ids.clone()))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = model.training_step((img, ids.clone()))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    value = batch * steps / dt
    rec = {"workload": "BASELINE cfg %d: %s + ArcFace (PartialFC rate 1.0), %d ids, B=%d, %dx%d" % (
               5 if network.startswith("AlterNet") else 4, network, classes, batch, a.img_size, a.img_size),
           "dtype": "fp8-weights" if fp8 else "bf16", "value": round(value, 1), "unit": "imgs/sec", "steps": steps, "warmup": warmup,
           "ms_per_step": round(dt / steps * 1e3, 3), "final_loss": round(float(out["loss"]), 4),
           "step_frac": round(value * (FLOP_IMG[network] + 6.0 * 512 * classes) / 1e12 / BF16_DENSE_PEAK_TFLOPS, 4),
           "step_frac_peak": "bf16 dense MFMA %.1f TFLOP/s (also for the fp8 run: its backward is bf16)" % BF16_DENSE_PEAK_TFLOPS}
    del model, img, ids
    torch.cuda.empty_cache()
    return rec


DUMP_BYTES = 60 << 20          # --dump-outputs stays under 64 MB in all: the array data, with room for the .npy headers


def dump_outputs(path, model, loss):
    """Write what one training step hands its caller -- the loss, and the model state it leaves behind (encoder.<key>: parameters
    and BatchNorm statistics; head.<key>: class centres) -- to path/<name>.npy, floating tensors as float32, integer ones as float64.
    With PartialFC sampling (rate < 1) head.weight is the full class-centre buffer, into which the sampled rows are written back only
    when the next step samples (PartialFC.update), so the rows the step itself updated are dumped as head.weight_activated.  Every
    array gets an equal share of DUMP_BYTES; a larger tensor is reduced to a fixed sample of distinct positions drawn from a generator
    seeded by the tensor's name, so that another build of the project samples the same positions."""
    import zlib
    import numpy as np
    os.makedirs(path, exist_ok=True)
    state = [(part + "." + k, v.detach()) for part, mod in (("encoder", model.encoder), ("head", model.loss))
             for k, v in mod.state_dict().items() if v.numel()]
    if getattr(model.loss, "sample_rate", 1.0) < 1:
        state.append(("head.weight_activated", model.loss.weight_activated.detach()))
    share = DUMP_BYTES // (len(state) + 1)
    np.save(os.path.join(path, "loss.npy"), loss.detach().float().cpu().numpy())
    total = 0
    for k, v in state:
        fp = v.is_floating_point()
        flat, cap = v.reshape(-1), share // (4 if fp else 8)
        if flat.numel() > cap:
            idx = np.sort(np.random.default_rng(zlib.crc32(k.encode())).choice(flat.numel(), cap, replace=False))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        a = flat.to(torch.float32 if fp else torch.float64).cpu().numpy()
        np.save(os.path.join(path, k + ".npy"), a)
        total += a.nbytes
    log("outputs of the last timed step: %d arrays, %.1f MB in %s" % (len(state) + 1, total / 2**20, path))


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def self_launch(n):
    """`python bench.py --gpus N` without a launcher (where the reference does mp.spawn(train, nprocs=world_size), main/main.py:255-259):
    start N ranks of this script under torch.distributed.run as a CHILD process and return its exit code.  This process has made no HIP
    call at this point (importing torch does not initialise the device) and it never replaces itself: the ranks inherit stdout, so rank 0's
    JSON line is this command's output."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "4")
    print("[bench] starting %d ranks: %s" % (n, " ".join(cmd)), file=sys.stderr, flush=True)
    return subprocess.run(cmd, env=env).returncode


def log(msg):
    if int(os.environ.get("RANK", "0")) == 0:
        print("[bench %7.1fs] %s" % (time.time() - T_START, msg), file=sys.stderr, flush=True)


T_START = time.time()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="images per GPU (default 512; 256 for AlterNet50 @192, cfg 5)")
    ap.add_argument("--classes", type=int, default=NUM_CLASSES)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--network", default="ResNet50",
                    help="ResNet50 (headline, BASELINE cfg 2/3), Swin34 (cfg 4) or AlterNet50 (cfg 5 geometry: 192x192, bf16)")
    ap.add_argument("--graph", action="store_true",
                    help="replay the step as one HIP graph (default: eager launches; eager is GPU-bound at B=512 and "
                         "lets the side-stream weight-gradient GEMMs overlap the main stream)")
    ap.add_argument("--no-graph", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--fp8", action="store_true",
                    help="BASELINE cfg 5: forward convolutions / linears with >= 128 input channels on the fp8 MFMA path")
    ap.add_argument("--no-extra", action="store_true", help="skip the cfg 4 / cfg 5 runs that follow the headline measurement")
    ap.add_argument("--dist-path", action="store_true",
                    help="rehearse the N>1 code path (RCCL group, DDP wrap, PartialFC rate 0.1) in a 1-rank group")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write the last one's loss and the model state it left to DIR/<name>.npy (rank 0)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    args.img_size = 192 if args.network.startswith("AlterNet") else 112
    if args.batch is None:
        args.batch = 256 if args.network.startswith("AlterNet") else BATCH

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus))               # `python bench.py --gpus N` starts its own ranks (reference main/main.py:255-259)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, "WORLD_SIZE=%d but --gpus %d" % (world, args.gpus)
    # rehearsal hook (one-GPU boxes): FRHIP_BENCH_BACKEND=gloo runs the N > 1 code path with every rank on cuda:0
    backend = os.environ.get("FRHIP_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local = 0
    torch.cuda.set_device(local)
    # gloo's C++ side prints a connection banner on STDOUT: keep stdout for the one JSON line (fd 1 points at stderr during the rendezvous)
    sys.stdout.flush()
    saved_fd = os.dup(1)
    os.dup2(2, 1)
    try:
        if backend != "nccl" and world > 1:
            dist.init_process_group(backend)
        elif world > 1 or args.dist_path:
            if world == 1:
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                os.environ.setdefault("MASTER_PORT", str(free_port()))
                os.environ.setdefault("RANK", "0")
                os.environ.setdefault("WORLD_SIZE", "1")
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("gloo", init_method="file://" + os.path.join(tempfile.mkdtemp(), "pg"),
                                    rank=0, world_size=1)
    finally:
        os.dup2(saved_fd, 1)
        os.close(saved_fd)

    import __graft_entry__ as ge
    if rank == 0:
        ge.build()
    if world > 1:
        dist.barrier()
    from frhip import ops
    from model.FR_PartialFC import Model

    log("library built/loaded")
    conf = make_conf(args, local, world)
    conf.frhip_fp8 = bool(args.fp8)
    if args.dist_path:
        conf.sample_rate, conf.force_ddp = 0.1, True
    torch.manual_seed(1234 + rank)
    model = Model(conf, None, "train")
    model.sync_loss = False
    gen = torch.Generator().manual_seed(1234 + rank)
    img = torch.randn((args.batch, 3, args.img_size, args.img_size), generator=gen).clamp_(-1, 1).cuda()
    ids = torch.randint(0, args.classes, (args.batch,), generator=gen).cuda()
    meter = ConvMeter(ops)
    log("model + synthetic batch ready (B=%d, classes=%d)" % (args.batch, args.classes))

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    use_graph = world == 1 and args.graph and not args.dist_path
    meter.collect = True
    model.training_step((img, ids.clone()))          # eager; also records the conv launch list for the probe
    meter.collect = False
    torch.cuda.synchronize()
    log("eager step done (%d conv launches recorded)" % len(meter.calls))
    if use_graph:
        model.capture_training_step((img, ids))
        log("step captured into a HIP graph")
    for i in range(args.warmup):
        model.training_step((img, ids.clone()))
    torch.cuda.synchronize()
    log("warm-up done")
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = model.training_step((img, ids.clone()))
    sync()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:              # before the instrumented steps below move the model on
        dump_outputs(args.dump_outputs, model, out["loss"])
    # Dominant-kernel durations INSIDE running steps: the same loop again, now with two HIP events around every conv launch.
    # Kept out of the timed region above: the ~230 event records per step cost 0.6-0.7 ms of a 27-ms step (measured), which
    # would be charged to `value`; the instrumented steps run right behind the timed ones in the same process and state.
    instep = rank == 0 and not use_graph and os.environ.get("FRHIP_BENCH_INSTEP", "1") == "1"
    in_steps = min(args.steps, 10)
    in_n = in_ms = in_fl = f8_n = f8_ms = f8_fl = 0
    in_dt = None
    if instep:
        meter.start_instep()
    if world > 1 or instep:
        sync()
        t1 = time.perf_counter()
        for _ in range(in_steps):
            model.training_step((img, ids.clone()))
        sync()
        in_dt = time.perf_counter() - t1
    if instep:
        f8_n, f8_ms, f8_fl = meter.stop_instep8()
        in_n, in_ms, in_fl = meter.stop_instep()
    t = torch.tensor([dt], dtype=torch.float64, device="cuda")
    ones = torch.ones(1, dtype=torch.float32, device="cuda")
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.all_reduce(ones, op=dist.ReduceOp.SUM)      # every rank of the group (RCCL for the default backend) adds one
    dt = float(t.item())
    n_ranks = int(round(float(ones.item())))             # n_gpus of the JSON line = ranks the collective really reached
    assert n_ranks == dist.get_world_size() == world, (n_ranks, dist.get_world_size(), world)
    loss = float(out["loss"])
    log("timed region: %.3f s for %d steps" % (dt, args.steps))

    if rank == 0:
        n, ms, fl = meter.measure()
        probe = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        # dominant-kernel roofline: measured INSIDE the timed steps (the weight-gradient side stream shares the chip with these
        # launches there); the back-to-back re-issue of the same launch list after the timed region is kept as `probe`
        if in_n:
            launches, achieved = in_n // in_steps, in_fl / (in_ms * 1e-3) / 1e12
            avg_us, flop_per_launch = in_ms * 1e3 / in_n, in_fl / in_n
        else:
            launches, achieved, avg_us, flop_per_launch = n, probe, ms * 1e3 / max(n, 1), fl / max(n, 1)
        traffic, traffic_src = pmc_traffic(args)
        flop_img = FLOP_IMG.get(args.network)
        value = args.batch * world * args.steps / dt
        step_frac = None
        if flop_img is not None:
            head_flop = 6.0 * 512 * (args.classes * conf.sample_rate if conf.sample_rate < 1 else args.classes)
            step_frac = round(value / world * (flop_img + head_flop) / 1e12 / BF16_DENSE_PEAK_TFLOPS, 4)
        line = {
            "metric": "train imgs/sec IR-50-layout ResNet50 + ArcFace/PartialFC head, 112x112" if args.network == "ResNet50"
                      else "train imgs/sec %s + ArcFace/PartialFC head, %dx%d" % (args.network, args.img_size, args.img_size),
            "value": round(value, 1), "unit": "imgs/sec", "n_gpus": n_ranks,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "fp8-weights" if args.fp8 else "bf16", "data": "synthetic",
            "config": {"workload": "BASELINE cfg %d: %s+%s, %d ids, B=%d/GPU, SGD "
                                   "mom 0.9 wd 5e-4, s=30 m=0.35" % ((2 if world == 1 else 3) if args.network == "ResNet50" else (5 if args.network.startswith("AlterNet") else 4),
                                                                     "ResNet50([3,4,14,4] BasicBlock)" if args.network == "ResNet50" else args.network,
                                                                     "ArcFace (PartialFC rate 1.0)" if conf.sample_rate >= 1 else "ArcFace (PartialFC rate %.1f)" % conf.sample_rate,
                                                                     args.classes, args.batch),
                       "global_batch": args.batch * world, "parallelism": "dp%d+class-shard%d" % (world, world),
                       "launch": "hip-graph" if use_graph else "eager",
                       "collective_backend": dist.get_backend() if world > 1 else "none (1 rank)"},
            "final_loss": round(loss, 4),
            "roofline": {"bound": "mfma", "achieved": round(achieved, 1), "peak": BF16_DENSE_PEAK_TFLOPS,
                         "unit": "TFLOP/s", "frac": round(achieved / BF16_DENSE_PEAK_TFLOPS, 4), "traffic": traffic,
                         "traffic_source": traffic_src,
                         "kernel": "frhip::halo_kernel<bf16> + frhip::halo_wide_kernel + frhip::nt_kernel<bf16> (conv forward + data-gradient implicit GEMM)",
                         "measured": ("HIP events around every launch inside %d further steps of the same loop, run right behind the timed "
                                      "region (%.3f ms per instrumented step: the event records themselves cost ~0.6 ms)"
                                      % (in_steps, in_dt / in_steps * 1e3)) if in_n else "back-to-back re-issue",
                         "launches": launches, "avg_launch_us": round(avg_us, 2), "flop_per_launch": round(flop_per_launch),
                         "probe": {"achieved": round(probe, 1), "frac": round(probe / BF16_DENSE_PEAK_TFLOPS, 4),
                                   "what": "the same launch list re-issued back to back after the timed region (nothing else on the chip)"},
                         "step_frac": step_frac},
        }
        n_xf = getattr(meter, "instep_xf", 0) // max(in_steps, 1) if in_n else 0
        if n_xf:
            line["roofline"]["note"] = ("%d of the %d calls (conv2 of the stride-1 blocks) also form relu(bn1(y1)) in their operand path and write it "
                                        "out (FRHIP_FUSE_BN1=3, the default): the BatchNorm-apply pass they absorb is in their duration, not in "
                                        "their FLOP -- the step is 0.23 ms shorter for it and this fraction 0.017 lower than with FRHIP_FUSE_BN1=0"
                                        % (n_xf, launches))
        if f8_n:
            f8 = f8_fl / (f8_ms * 1e-3) / 1e12
            line["roofline_fp8"] = {"bound": "mfma", "achieved": round(f8, 1), "peak": 2 * BF16_DENSE_PEAK_TFLOPS, "unit": "TFLOP/s",
                                    "frac": round(f8 / (2 * BF16_DENSE_PEAK_TFLOPS), 4), "traffic": None,
                                    "kernel": "frhip::halo8_kernel (3x3 stride 1: v_mfma_f32_16x16x32_fp8_fp8) + frhip::nt8_kernel (other convs: v_mfma_scale_f32_16x16x128_f8f6f4), fp8 e4m3 x e4m3 forward convolutions",
                                    "launches": f8_n // in_steps, "avg_launch_us": round(f8_ms * 1e3 / f8_n, 2)}
        if world == 1 and not args.no_cpu_baseline and args.network == "ResNet50":
            line["cpu_baseline"] = cpu_baseline(args.classes)
            line["cpu_baseline_cfg1"] = cpu_baseline_cfg1()
        # BASELINE cfg 4 / cfg 5 in the same process, after (and outside) the headline's timed region; the headline fields above are
        # final at this point.  Only in the plain headline run: N = 1, ResNet50, default batch, eager.
        if (world == 1 and args.network == "ResNet50" and args.batch == BATCH and not args.dist_path and not use_graph and not args.fp8
                and not args.no_extra and os.environ.get("FRHIP_BENCH_EXTRA", "1") == "1"):
            del model, out
            torch.cuda.empty_cache()
            extras = []
            for net, b, f8 in (("Swin34", 512, False), ("AlterNet50", 256, False), ("AlterNet50", 256, True)):
                try:
                    extras.append(extra_config(net, b, f8, args.classes))
                    log("extra config %s%s: %.1f img/s" % (net, " fp8" if f8 else "", extras[-1]["value"]))
                except Exception as e:       # the headline line must still be printed
                    extras.append({"workload": "%s B=%d%s" % (net, b, " fp8" if f8 else ""), "error": repr(e)[:300]})
            line["extra_configs"] = extras
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
