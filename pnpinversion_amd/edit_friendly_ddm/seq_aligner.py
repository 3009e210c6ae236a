"""API-compatibility alias of models/edit_friendly_ddm/seq_aligner.py (identical to the P2P copy); the implementation is p2p/token_align.py."""
from ..p2p.token_align import (get_mapper, get_refinement_mapper, get_replacement_mapper, get_replacement_mapper_,  # noqa: F401
                               get_word_inds)
