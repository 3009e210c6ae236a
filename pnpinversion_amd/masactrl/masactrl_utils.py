"""AttentionBase / regiter_attention_editor_diffusers with the names of models/masactrl/masactrl_utils.py:14-41,85-144.
On the native pipeline an "attention editor" is not a Python callback inside the UNet: it is translated into the kernel-side
descriptor (engine.MasaCtrlTables -> pnpi_ctrl_desc kind 2); `regiter_attention_editor_diffusers` just hands it to the model.
A mask-guided editor also uploads its masks (pnpi_masa_set_masks); registering any other editor clears them."""


class AttentionBase:
    """masactrl_utils.py:14-41: the identity editor (plain attention)."""

    def __init__(self):
        self.cur_step = 0
        self.num_att_layers = -1
        self.cur_att_layer = 0

    def after_step(self):
        pass

    def reset(self):
        self.cur_step = 0
        self.cur_att_layer = 0

    def tables(self):
        return None


class ForeignMasaCtrlAdapter:
    """An object of the reference's OWN MutualSelfAttentionControl / MutualSelfAttentionControlMask (models/masactrl/masactrl.py: no
    `.tables()`): the descriptor is read off its attributes (step_idx, layer_idx, mask_s, mask_t), the way foreign Prompt-to-Prompt
    controllers are read; the step bookkeeping stays on the wrapped object."""

    def __init__(self, wrapped):
        self.__dict__["wrapped"] = wrapped
        self.__dict__["_tables"] = _tables_from_attributes(wrapped)

    def __getattr__(self, name):
        return getattr(self.wrapped, name)

    def __setattr__(self, name, value):
        setattr(self.wrapped, name, value)

    def tables(self):
        return self._tables


def _tables_from_attributes(ed):
    from ..engine import MasaCtrlMaskTables, MasaCtrlTables
    layer_idx, step_idx = [int(x) for x in ed.layer_idx], [int(x) for x in ed.step_idx]
    if type(ed).__name__ == "MutualSelfAttentionControlMask":
        ms, mt = getattr(ed, "mask_s", None), getattr(ed, "mask_t", None)
        if ms is not None and mt is not None:
            return MasaCtrlMaskTables(layer_idx=layer_idx, step_idx=step_idx, mask_s=ms, mask_t=mt)
        if ms is not None or mt is not None:
            raise ValueError("MutualSelfAttentionControlMask with only one of mask_s / mask_t is not built (the reference then masks the "
                             "keys without blending, or blends unmasked passes)")
    return MasaCtrlTables(layer_idx=layer_idx, step_idx=step_idx)


def adapt_foreign_editor(editor):
    """this package's editors (they carry `.tables()`) unchanged; the reference's two classes wrapped; anything else is refused -- the
    native UNet cannot run an arbitrary Python attention forward."""
    if editor is None or hasattr(editor, "tables"):
        return editor
    name = type(editor).__name__
    if name == "AttentionBase":
        return ForeignMasaCtrlAdapterNoEdit(editor)
    if name in ("MutualSelfAttentionControl", "MutualSelfAttentionControlMask"):
        return ForeignMasaCtrlAdapter(editor)
    raise TypeError("attention editor %s has no kernel descriptor: MutualSelfAttentionControl and MutualSelfAttentionControlMask "
                    "(this package's or the reference's) are built" % name)


class ForeignMasaCtrlAdapterNoEdit(ForeignMasaCtrlAdapter):
    """the reference's identity editor"""

    def __init__(self, wrapped):
        self.__dict__["wrapped"] = wrapped
        self.__dict__["_tables"] = None


def regiter_attention_editor_diffusers(model, editor: AttentionBase):
    """masactrl_utils.py:85-144 (the reference hooks the 32 `Attention` modules; the count is what it stores).  Registering uploads a
    mask-guided editor's masks to the model's context and clears the masks of an earlier editor otherwise."""
    editor = adapt_foreign_editor(editor)
    model.masactrl_editor = editor
    editor.num_att_layers = model.engine.cfg.n_attention_layers if hasattr(model.engine.cfg, "n_attention_layers") else 32
    tables = editor.tables()
    if getattr(tables, "mask_s", None) is not None:
        model.engine.masa_set_masks(tables.mask_s, tables.mask_t)
    else:
        model.engine.masa_set_masks()
