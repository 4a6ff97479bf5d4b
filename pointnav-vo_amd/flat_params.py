"""One flat parameter store for a train step: the module's parameters, their gradients and Adam's two moments as four flat float32
buffers, with the parameters (and their .grad) re-pointed at views of them.

VOTrainStep (train.py) and PolicyTrainStep (ppo.py) each hold one `FlatParams`; the HIP kernels read and write the buffers through the
table `toc` (name, offset, shape per parameter), torch sees the same memory through the module.  The layout is fixed at construction:
parameter i starts at the end of parameter i - 1 rounded up to `align` floats, the gaps hold zeros, and `tail` more floats follow the
last parameter in `flat` and `grad` for the owner's own use (ppo.py: the encoder handle's padded stem and unused head).

The owner's part.  The HIP Adam step writes `flat` and re-packs the kernels' operands itself.  Any other edit (load_state_dict on
resume, an in-place torch edit, a re-pointed p.data) lands in the module but not in the packed operands, so before every forward the
owner runs

    if not store.changed(): return
    store.realias(); <refresh its handle THREE times>; <synchronise the stream>; store.mark()

Three, because an outside edit can move a GroupNorm weight by any amount and the float16-piece range guard must be current at once:
the forward reads the bounds of the parameters TWO refreshes back (a fixed lag — fine for Adam's lr-sized steps, and the same on every
run and rank), and three refreshes fill that ring with the edited parameters' bounds.
"""
import ctypes as C

import torch


def flat_offsets(spec, align=4):
    """Layout of the flat buffers: (name, shape) in named_parameters() order -> ({name: (offset, numel)}, floats used).  Every tensor
    starts at a multiple of `align` floats (4: the policy's kernels read weight rows as 16-byte vectors); the gaps hold zeros."""
    offsets, off = {}, 0
    for name, shape in spec:
        n = 1
        for s in shape:
            n *= int(s)
        offsets[name] = (off, n)
        off = (off + n + align - 1) // align * align
    return offsets, off


class FlatParams:
    def __init__(self, named, device, align=1, tail=0):
        """named: the list(module.named_parameters()) the caller froze (order = layout order)."""
        self.named = list(named)
        self.offsets, self.n_params = flat_offsets([(n, tuple(p.shape)) for n, p in self.named], align)
        n = self.n_params
        self.flat = torch.zeros(n + tail, device=device, dtype=torch.float32)     # zeros: the gaps and the tail
        self.grad = torch.zeros(n + tail, device=device, dtype=torch.float32)
        self.exp_avg = torch.zeros(n, device=device, dtype=torch.float32)
        self.exp_avg_sq = torch.zeros(n, device=device, dtype=torch.float32)
        self._params = [p for _, p in self.named]
        self._toc = None
        with torch.no_grad():
            for name, p in self.named:
                self._view(self.flat, name, p).copy_(p.detach())
                self._alias(name, p)
        self.mark()

    def _view(self, buf, name, p):
        off, k = self.offsets[name]
        return buf[off:off + k].view(p.shape)

    def _alias(self, name, p):
        p.data = self._view(self.flat, name, p)           # the module's parameters alias the flat buffer
        p.grad = self._view(self.grad, name, p)

    @property
    def toc(self):
        """The pnvo_tensor_desc table of the layout (built once, kept: the library reads the names through it)."""
        if self._toc is None:
            from . import _lib
            self._toc = _lib.make_toc([(n, self.offsets[n][0], tuple(p.shape)) for n, p in self.named])
        return self._toc

    # ------------------------------------------------------------------ edits from outside the HIP Adam step
    def _sig(self):
        return tuple([(p.data_ptr(), p._version) for p in self._params])

    def changed(self):
        """Whether a parameter was written in place or re-pointed since mark() (load_state_dict on resume, a torch edit), by torch's
        version counter: a write through `p.data` (p.data.add_(1)) does not count there and is not seen."""
        return self._sig() != self._marked

    def realias(self):
        """A parameter the caller re-pointed (p.data = other): its value is copied into the flat buffer and the alias restored.  In-place
        edits already are in the flat buffer."""
        with torch.no_grad():
            for name, p in self.named:
                view = self._view(self.flat, name, p)
                if p.data_ptr() != view.data_ptr():
                    view.copy_(p.detach())
                    self._alias(name, p)

    def mark(self):
        self._marked = self._sig()

    # ------------------------------------------------------------------ Adam
    def adam_state_dict(self, names, step_count, lr, betas, eps):
        """Optimizer state in torch.optim.Adam's layout over the parameters `names`, in that order: per-parameter step / exp_avg /
        exp_avg_sq and one param group."""
        shapes = {n: p.shape for n, p in self.named}
        state = {}
        for i, n in enumerate(names):
            off, k = self.offsets[n]
            state[i] = {"step": torch.tensor(float(step_count)),
                        "exp_avg": self.exp_avg[off:off + k].view(shapes[n]).clone(),
                        "exp_avg_sq": self.exp_avg_sq[off:off + k].view(shapes[n]).clone()}
        group = {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": 0, "amsgrad": False, "params": list(range(len(state)))}
        return {"state": state, "param_groups": [group]}

    def load_adam_state_dict(self, sd, names):
        """-> (step_count, param group).  A parameter without state gets zero moments; the ranges of parameters outside `names` stay."""
        steps = set()
        with torch.no_grad():
            for i, n in enumerate(names):
                off, k = self.offsets[n]
                st = sd["state"].get(i)
                if st is None:
                    self.exp_avg[off:off + k].zero_()
                    self.exp_avg_sq[off:off + k].zero_()
                else:
                    self.exp_avg[off:off + k].copy_(st["exp_avg"].reshape(-1))
                    self.exp_avg_sq[off:off + k].copy_(st["exp_avg_sq"].reshape(-1))
                    steps.add(int(st["step"]))
        if len(steps) > 1:
            raise ValueError("per-parameter Adam step counts differ; the HIP Adam keeps one step count for all parameters")
        return (steps.pop() if steps else 0), sd["param_groups"][0]

    def adam_step(self, ranges, lr, betas, eps, step_count, stream):
        """One pnvo_adam_step per flat range (lo, hi) on `stream` (a c_void_p)."""
        from . import _lib
        for lo, hi in ranges:
            ptr = lambda t: C.c_void_p(t.data_ptr() + 4 * lo)
            _lib.check(_lib.lib.pnvo_adam_step(ptr(self.flat), ptr(self.grad), ptr(self.exp_avg), ptr(self.exp_avg_sq), hi - lo, lr,
                                               betas[0], betas[1], eps, step_count, stream))
