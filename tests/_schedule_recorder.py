"""Records what a train step hands to the GPU and to the process group, in host call order, as short strings: graph
replays (named by the order in which the graphs were captured), the dense all-reduces, the all-to-alls, the explicit
lookup step's stages, the pipeline's input dist and the optimizer step.  Everything is patched from outside, on the
classes and on the `torch.distributed` module, so the same recorder reads any version of the step that keeps those call
sites; it knows nothing of DLRMTrain.  tests/test_multirank_gpu.py compares a recording with
tests/golden/explicit_step_schedule.json (tests/golden/make_schedule_golden.py writes it): a refactor of the step that
moves, adds or drops a launch fails there instead of on the GPU.

Install it AFTER anything else that replaces `torch.distributed` functions (the rehearsal's host staging calls the real
all_to_all_single itself, which would otherwise be recorded a second time)."""
import contextlib

import torch
import torch.distributed as dist


@contextlib.contextmanager
def record_schedule():
    """`with record_schedule() as events:` — `events` is the growing list.  Graphs are numbered from 0 in the order of
    their `capture_begin` inside the context, so enter it before the model captures."""
    from torchrec_amd.distributed.embeddingbag import ExplicitLookupStep, ShardedEmbeddingBagCollection
    from torchrec_amd.distributed.train_pipeline import TrainPipelineSparseDist
    from torchrec_amd.optim.keyed import CombinedOptimizer

    events, undo, index = [], [], {}

    def patch(owner, name, describe):
        real = getattr(owner, name)

        def wrapper(*args, **kwargs):
            events.append(describe(*args, **kwargs))
            return real(*args, **kwargs)

        undo.append((owner, name, real))
        setattr(owner, name, wrapper)

    graph_cls = torch.cuda.CUDAGraph
    real_begin = graph_cls.capture_begin

    def numbered_begin(graph, *args, **kwargs):
        index[id(graph)] = (len(index), graph)  # (the graph itself is kept: its id is not reused while it lives)
        return real_begin(graph, *args, **kwargs)

    undo.append((graph_cls, "capture_begin", real_begin))
    graph_cls.capture_begin = numbered_begin
    patch(graph_cls, "replay", lambda graph: "replay g%s" % (index[id(graph)][0] if id(graph) in index else "?"))
    patch(dist, "all_reduce", lambda tensor, op=None, group=None, async_op=False:
          f"all_reduce numel={tensor.numel()} offset={tensor.storage_offset()} async={bool(async_op)}")
    patch(dist, "all_to_all_single", lambda output, input, output_split_sizes=None, input_split_sizes=None, group=None,
          async_op=False: f"all_to_all_single numel={input.numel()} async={bool(async_op)}")
    patch(dist, "all_to_all", lambda output_tensor_list, input_tensor_list, group=None, async_op=False:
          f"all_to_all numel={sum(t.numel() for t in input_tensor_list)} async={bool(async_op)}")
    patch(ExplicitLookupStep, "finish", lambda step: "lookup.finish")
    patch(ExplicitLookupStep, "finish_half", lambda step, h: f"lookup.finish_half {h}")
    patch(ExplicitLookupStep, "start_backward", lambda step, grad_out: "lookup.start_backward")
    patch(ExplicitLookupStep, "start_backward_half", lambda step, h, grad_rows, grad_out=None:
          f"lookup.start_backward_half {h}")
    patch(ExplicitLookupStep, "finish_backward", lambda step: "lookup.finish_backward")
    patch(ExplicitLookupStep, "discard", lambda step: "lookup.discard")
    patch(ShardedEmbeddingBagCollection, "compute_explicit", lambda ebc, dist_input, prefetched=False:
          f"compute_explicit prefetched={bool(prefetched)}")
    patch(TrainPipelineSparseDist, "_start_data_dist", lambda pipe, batch: "start_data_dist")
    patch(CombinedOptimizer, "step", lambda opt, closure=None: "optimizer.step")
    try:
        yield events
    finally:
        for owner, name, real in reversed(undo):
            setattr(owner, name, real)
