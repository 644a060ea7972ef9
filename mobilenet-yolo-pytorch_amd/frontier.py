"""Which part of the graph a backward pass has to visit when some parameters are frozen (`requires_grad == False`) and which
BatchNorm modes a plan can honour.  Pure functions of (graph, names): no device, no library, no torch.

A node needs a backward call only if a loss depends on it and it owns a trainable parameter or some node upstream of it (towards
the image) does; the gradient of a value is needed under exactly the same condition on its producer.  So one set describes both:
`Frontier.grad_values`, the ids of the values whose gradient the backward list forms.  A node is kept iff its output is in the set;
a kept node emits the gradient of an input iff that input is in the set.  Every consumer of a value in the set is kept (the value
is upstream of it), so each gradient the list forms is complete.
"""
from ._lib import MnyError


def node_params(nd):
    """Parameter names of a node, in the order the gradient arena lists them."""
    names = []
    if nd.conv:
        names.append(nd.conv + ".weight")
        if nd.bias:
            names.append(nd.conv + ".bias")
    if nd.bn:
        names += [nd.bn + ".weight", nd.bn + ".bias"]
    return names


def loss_outputs(g):
    return list(g.outputs) + ([g.seg_out] if g.seg_out is not None else [])


def live_values(g):
    """ids of the values a loss (or detection output) depends on."""
    live, stack = set(), loss_outputs(g)
    while stack:
        v = stack.pop()
        if v.node is None or v.id in live:
            continue
        live.add(v.id)
        stack.extend(v.node.ins)
    return live


class Frontier:
    """grad_values: ids of the values whose gradient is formed (== outputs of the nodes that get a backward call);
    order: those nodes in backward order; grad_params: the trainable parameter names in arena (production) order — a module applied
    twice has two nodes in `order` and one slot."""

    def __init__(self, g, frozen=()):
        frozen = frozenset(frozen)
        self.frozen = frozen
        live = live_values(g)
        up = {}                                   # value id -> a trainable parameter sits at or upstream of its producer
        for nd in g.nodes:                        # forward (topological) order
            up[nd.out.id] = (any(nm not in frozen for nm in node_params(nd)) or any(up.get(v.id, False) for v in nd.ins))
        self.grad_values = {vid for vid, u in up.items() if u and vid in live}
        self.order = [nd for nd in reversed(g.nodes) if nd.out.id in self.grad_values]
        self.grad_params = []
        seen = set()
        for nd in self.order:
            for nm in node_params(nd):
                if nm not in seen and nm not in frozen:
                    seen.add(nm)
                    self.grad_params.append(nm)

    def needs_grad(self, v):
        """Is the gradient of value `v` formed?  For a node's output: does the node get a backward call?"""
        return v.id in self.grad_values


def bn_names(g):
    out, seen = [], set()
    for nd in g.nodes:
        if nd.bn and nd.bn not in seen:
            seen.add(nd.bn)
            out.append(nd.bn)
    return out


def check_bn_modes(g, fr, bn_eval):
    """A plan on batch statistics (some BatchNorm module in training mode) takes eval-mode BatchNorms only below the frontier, where
    they are constants of the step.  Raises MnyError naming the first eval-mode module the backward pass would have to go through."""
    if not bn_eval:
        return
    for nd in g.nodes:
        if nd.bn in bn_eval and fr.needs_grad(nd.out):
            raise MnyError("BatchNorm module %s is in eval mode on the gradient path while others are in training mode: mixed BatchNorm "
                           "modes are supported only below the frozen frontier (freeze everything up to it, or put every BatchNorm "
                           "in eval mode)" % nd.bn)


def check_fused_pair(members, bn_eval, what):
    """members: the BatchNorm module names of one fused multi-BatchNorm unit; they must agree on their mode."""
    modes = {nm in bn_eval for nm in members}
    if len(modes) > 1:
        odd = [nm for nm in members if nm in bn_eval]
        raise MnyError("BatchNorm module %s is in eval mode but shares the fused %s unit with %s in training mode: the members of a fused "
                       "unit must agree" % (odd[0], what, ", ".join(nm for nm in members if nm not in bn_eval)))
