"""models/edit_friendly_ddm/ptp_utils.py: the pieces the editing script uses.  The word-index and time-word tables are the same functions
as the P2P copy's (they differ only in type hints), so they are shared."""
from ..p2p.attention_control import register_attention_control  # noqa: F401
from ..p2p.token_align import get_word_inds  # noqa: F401
from ..utils.utils import get_time_words_attention_alpha, update_alpha_time_word  # noqa: F401
