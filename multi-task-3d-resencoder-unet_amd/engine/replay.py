"""What the two replay backends of a plan's run side (launch programs, HIP graphs: engine/plan.py) have in common, and the
tensor normalisation every boundary of the run side uses.  Pure functions: the plan keeps the state and supplies the backend."""
import torch


def as_f32(t):
    """`t` as the kernels read a boundary tensor: detached, fp32, contiguous.  Returns (tensor, copied?): a copy is a temporary,
    whose address no recorded program may keep."""
    t = t.detach()
    if t.dtype != torch.float32 or not t.is_contiguous():
        return t.float().contiguous(), True
    return t, False


def ladder(states, slot, key, ptrs, body, record, replay):
    """The replay ladder of one launch list: run `body` eagerly twice (lazy allocations, workspace growth, first-use attributes),
    then `record(st, body)` once -- it runs body, leaves its result in st["result"] and returns the recording, kept as
    st[slot] -- and `replay(st)` ever after.  `ptrs` (the parameter addresses) differing from those of the recording starts the
    ladder over: the parameters were re-allocated.  Returns (st, "eager" | "record" | "replay")."""
    st = states.setdefault(key, {"calls": 0})
    if st.get(slot) is not None and st["ptrs"] != ptrs:
        st.clear()
        st["calls"] = 0
    if st.get(slot) is not None:
        replay(st)
        return st, "replay"
    if st["calls"] < 2:
        st["calls"] += 1
        st["result"] = body()
        return st, "eager"
    st[slot] = record(st, body)
    st["ptrs"] = ptrs
    return st, "record"


def unalias_grads(params, aliased):
    """Gradient accumulation over persistent gradient storage: autograd normally adopts the tensors a backward returns as
    `.grad`; a `.grad` the caller kept whose address `aliased(ptr)` says is about to be overwritten is moved out of the way."""
    for p in params:
        gr = p.grad
        if gr is not None and aliased(gr.data_ptr()):
            p.grad = gr.clone()


def fresh_views(grads):
    """fresh tensor objects over persistent storage (autograd adopts a gradient only if nobody else holds it)"""
    return [t.detach() if t is not None else None for t in grads]
