"""Prompt-to-Prompt controllers of models/edit_friendly_ddm/ptp_classes.py, declarative form (see p2p/attention_control.py).

They differ from the P2P copy in three ways, all reproduced here:
  * constructors take `model=` (tokenizer and device are read from it, :182-199);
  * self-attention is replaced only at sites with <= 16**2 tokens (:139), not 32**2: ControllerTables(self_max_tokens=256);
  * LOW_RESOURCE = True (:7): the unconditional and the conditional batch are separate UNet calls and only the second one -- the
    conditional rows [cond_src, cond_tgt] -- is edited, with cur_step counting the pass's own steps.  That is the row layout of the
    library's controller descriptor, so nothing else changes.
This copy's LocalBlend (:20-45) blends from step 0 and normalises per image over its full map, unlike the P2P copy the kernels implement;
the editing script does not use it, so it is refused rather than approximated."""
from ..p2p import attention_control as _p2p

LOW_RESOURCE = True
MAX_NUM_WORDS = 77
SELF_MAX_TOKENS = 16 ** 2


class LocalBlend:
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("edit_friendly_ddm LocalBlend is not supported: it blends from the first step and normalises differently "
                                  "from the Prompt-to-Prompt LocalBlend the edit kernels implement (ptp_classes.py:20-45)")


def _check(local_blend, model):
    if local_blend is not None:
        raise NotImplementedError("edit_friendly_ddm controllers with a LocalBlend are not supported (see LocalBlend)")
    if model is None:
        raise TypeError("edit_friendly_ddm controllers need model= (its tokenizer builds the token tables)")


class EmptyControl(_p2p.EmptyControl):
    pass


class AttentionStore(_p2p.AttentionStore):
    pass


class _EditTables:
    def tables(self):
        t = super().tables()
        t.self_max_tokens = SELF_MAX_TOKENS
        return t


class AttentionReplace(_EditTables, _p2p.AttentionReplace):
    def __init__(self, prompts, num_steps, cross_replace_steps, self_replace_steps, local_blend=None, model=None):
        _check(local_blend, model)
        super().__init__(prompts, num_steps, cross_replace_steps, self_replace_steps, None, tokenizer=model.tokenizer, device=model.device)


class AttentionRefine(_EditTables, _p2p.AttentionRefine):
    def __init__(self, prompts, num_steps, cross_replace_steps, self_replace_steps, local_blend=None, model=None):
        _check(local_blend, model)
        super().__init__(prompts, num_steps, cross_replace_steps, self_replace_steps, None, tokenizer=model.tokenizer, device=model.device)


class AttentionReweight:
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("edit_friendly_ddm AttentionReweight is not supported (the editing script does not use it)")
