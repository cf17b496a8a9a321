"""Bit-level A/B of every entry point of csrc/rx_instnorm.hip, rx_head.hip and rx_se.hip between two builds of the library.

    python scripts/ab_instnorm_family.py --base <librxunet.so of the parent> [--new <other build>] [--timeout 300]

One fresh child process per library (RX_LIBRARY selects the build), each under its own `timeout`; the run stops at the first child
that fails.  A child runs a fixed list of calls on seeded inputs and writes one SHA-256 per output tensor; the parent compares the
two lists and exits non-zero unless every hash is equal.  Shapes are the smallest that reach each reduction path (N = 2):
    C=32 4^3      single launch, 32 channels per workgroup
    C=32 8^3      single launch, 8 channels per workgroup in the 16-bit types
    C=64 5x12x16  three launches, shuffle rows
    C=96 5x12x16  three launches, LDS rows (C/8 = 12 and C/4 = 24 divide neither into 64)
A pool stride that does not divide a shape, and the fused head forward where C/8 does not divide 64, are left out (the entry
points refuse them)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(32, (4, 4, 4)), (32, (8, 8, 8)), (64, (5, 12, 16)), (96, (5, 12, 16))]
N = 2


def child(path):
    sys.path.insert(0, ROOT)
    import torch
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import lib as L, ops

    gen = torch.Generator().manual_seed(1234)
    f32 = dict(dtype=torch.float32, device="cuda")
    hashes = []

    def put(label, *tensors):
        torch.cuda.synchronize()
        for i, t in enumerate(tensors):
            t = t.t if isinstance(t, ops.Act) else t
            raw = t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()
            hashes.append([f"{label}#{i}", hashlib.sha256(raw).hexdigest()])

    def rnd(*shape, k=1.0):
        return (torch.randn(*shape, generator=gen) * k).float().cuda()

    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        for c, dims in SHAPES:
            tag = f"{str(dtype)[6:]} c{c} {'x'.join(map(str, dims))}"
            act = lambda k=1.0: ops.Act(rnd(N, *dims, c, k=k).to(dtype))                      # noqa: E731
            like = lambda a, fill=None: ops.Act(torch.full_like(a.t, fill) if fill is not None else torch.zeros_like(a.t))  # noqa: E731
            y, res, g = act(2.0), act(), act(0.3)
            stats = torch.zeros((N, c, 2), **f32)
            ops.instnorm_stats(y, stats)
            put(f"{tag} stats", stats)
            keep = (torch.rand(N * c, generator=gen) > 0.3).float().cuda()
            masked = stats.clone()
            ops.instnorm_stats_mask(masked, keep)
            put(f"{tag} stats_mask", masked)
            csum = torch.zeros((c,), **f32)
            ops.channel_sum(y, csum)
            put(f"{tag} channel_sum", csum)
            out = like(y)
            for r in (None, res):
                o = like(y)
                ops.instnorm_act_fwd(y, stats, o, 0.01, r)
                put(f"{tag} act_fwd res={r is not None}", o)
                o2, s2 = like(y), torch.zeros_like(stats)
                ops.instnorm_fwd(y, s2, o2, 0.01, r)
                put(f"{tag} fwd res={r is not None}", o2, s2)
                if r is not None:
                    out = o
            m12 = rnd(N, c, 2, k=0.05)
            for mask, slope, oo in (("none", 1.0, None), ("out", 0.01, out), ("xhat", 0.01, None)):
                for dres_mode in ("absent", "written", "accumulated"):
                    for entry in ("bwd", "bwd_apply"):
                        dy = like(y)
                        dr = None if dres_mode == "absent" else like(y, 0.25)
                        if entry == "bwd":
                            ops.instnorm_act_bwd(g, y, stats, oo, dy, slope, dr, dres_mode == "accumulated")
                        else:
                            ops.instnorm_act_bwd_apply(g, y, stats, oo, dy, m12, slope, dr, dres_mode == "accumulated")
                        put(f"{tag} {entry} mask={mask} dres={dres_mode}", dy, *([dr] if dr is not None else []))
            for stride in (None, (2, 2, 2), (1, 2, 2)):
                if stride and any(d % s for d, s in zip(dims, stride)):
                    continue
                pdims = [d // s for d, s in zip(dims, stride)] if stride else None
                pool_dy = ops.Act(rnd(N, *pdims, c, k=0.3).to(dtype)) if stride else None
                dy, dr = like(y), like(y)
                ops.instnorm_act_bwd_res(g, y, stats, out, dy, dr, 0.01, pool_dy, stride or (1, 1, 1))
                put(f"{tag} bwd_res pool={stride}", dy, dr)
                if not stride:
                    continue
                for r in (None, res):
                    o, pooled = like(y), like(pool_dy)
                    ops.instnorm_act_pool_fwd(y, stats, o, pooled, stride, 0.01, r)
                    put(f"{tag} act_pool_fwd {stride} res={r is not None}", o, pooled)
                pooled, dx = like(pool_dy), like(y, 0.5)
                ops.avgpool_fwd(out, pooled, stride)
                ops.avgpool_bwd(pool_dy, dx, stride, True)
                put(f"{tag} avgpool {stride}", pooled, dx)
                ops.avgpool_bwd(pool_dy, dx, stride, False)
                put(f"{tag} avgpool_bwd {stride} acc=0", dx)
            V = dims[0] * dims[1] * dims[2]
            for K in (1, 3):
                hw, hb = rnd(K, c, k=0.2), rnd(K, k=0.1)
                dout = rnd(N, K, *dims, k=0.1)
                if dtype != torch.float32 and 64 % (c // 8) == 0:
                    for o in (like(y), None):
                        logits = torch.zeros((N, K, *dims), **f32)
                        ops.instnorm_act_head_fwd(y, stats, o, hw, hb, logits, L.RX_ACT_SIGMOID if K == 1 else L.RX_ACT_SOFTMAX, 0.01)
                        put(f"{tag} act_head_fwd K={K} out={o is not None}", logits, *([o] if o is not None else []))
                for slope in (0.01, 1.0):
                    for with_dw in (False, True):
                        dy = like(y)
                        dw, db = (torch.zeros((K, c), **f32), torch.zeros((K,), **f32)) if with_dw else (None, None)
                        ops.instnorm_act_bwd_head(dout, hw, y, stats, dy, slope, None, dw, db)
                        put(f"{tag} bwd_head K={K} slope={slope} dw={with_dw}", dy, *([dw, db] if with_dw else []))
                logits = torch.zeros((N, K, *dims), **f32)
                ops.head_fwd(out, hw, hb, logits, L.RX_ACT_NONE)
                dx, dw, db = like(y), torch.zeros((K, c), **f32), torch.zeros((K,), **f32)
                ops.head_bwd(dout, out, hw, dx, dw, db)
                put(f"{tag} head K={K} V={V}", logits, dx, dw, db)
            rd = 8
            for keep_x, with_se in ((0, True), (1, True), (1, False)):
                Ln = dims[2] if keep_x else 1
                mult, dadd, m12g = (torch.zeros((N, Ln, c), **f32), torch.zeros((N, Ln, c), **f32), torch.zeros((N, c, 2), **f32))
                se = pooled = hidden = gate = None
                grads = [None] * 4
                if with_se:
                    w = [rnd(rd, c, k=0.3), rnd(rd, k=0.1), rnd(c, rd, k=0.3), rnd(c, k=0.1)]
                    se = dict(w1=w[0], b1=w[1], w2=w[2], b2=w[3], rd=rd, keep_x=keep_x)
                    pooled, hidden, gate = torch.zeros((N, Ln, c), **f32), torch.zeros((N, Ln, rd), **f32), torch.zeros((N, Ln, c), **f32)
                    grads = [torch.zeros_like(t) for t in w]
                scale = torch.tensor([1.25, 0.0], **f32)
                ops.se_gate_fwd(y, stats, se, pooled, hidden, gate, mult, scale)
                put(f"{tag} se_gate_fwd keep_x={keep_x} se={with_se}", mult, *([pooled, hidden, gate] if with_se else []))
                for r in (None, res):
                    o = like(y)
                    ops.instnorm_gate_act_fwd(y, stats, mult, keep_x, o, 0.01, r)
                    put(f"{tag} gate_act_fwd keep_x={keep_x} se={with_se} res={r is not None}", o)
                for oo in (None, o):
                    sl = 0.01 if oo is not None else 1.0      # a gated block's mask needs the saved output: without it only slope 1
                    ops.se_gate_bwd(g, y, stats, oo, sl, se, pooled, hidden, gate, mult, dadd, m12g, *grads, path_scale=scale)
                    put(f"{tag} se_gate_bwd keep_x={keep_x} se={with_se} out={oo is not None}", dadd, m12g, *([t for t in grads] if with_se else []))
                    for dres_mode in ("absent", "written", "accumulated"):
                        dy = like(y)
                        dr = None if dres_mode == "absent" else like(y, 0.25)
                        ops.instnorm_gate_act_bwd(g, y, stats, oo, sl, mult, dadd, m12g, keep_x, dy, dr, dres_mode == "accumulated")
                        put(f"{tag} gate_act_bwd keep_x={keep_x} se={with_se} out={oo is not None} dres={dres_mode}", dy,
                            *([dr] if dr is not None else []))
    with open(path, "w") as f:
        json.dump(hashes, f)
    print(f"{len(hashes)} tensors hashed with {L.LIB_PATH}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base")
    ap.add_argument("--new", default=None, help="default: the library of this tree")
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    if not args.base:
        ap.error("--base is required")
    lists = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, lib in (("base", args.base), ("new", args.new)):
            env = dict(os.environ)
            env.pop("RX_LIBRARY", None)
            if lib:
                env["RX_LIBRARY"] = os.path.abspath(lib)
            out = os.path.join(tmp, name + ".json")
            rc = subprocess.call(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", out], env=env)
            if rc != 0:
                sys.exit(f"{name} ({lib or 'this tree'}): child exited with {rc}; stopping")
            with open(out) as f:
                lists.append(json.load(f))
    a, b = lists
    if [k for k, _ in a] != [k for k, _ in b]:
        sys.exit("the two builds produced different lists of tensors")
    bad = [ka for (ka, ha), (_, hb) in zip(a, b) if ha != hb]
    for k in bad:
        print("DIFFERENT:", k)
    print(f"{len(a)} tensors compared, {len(bad)} differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
