"""MI355X-native PairHMM likelihood engine, sort/mark-duplicate core and Smith-Waterman aligner.

Python is only a thin ctypes veneer over the C ABI of ``libmgx.so`` (include/mgx_pairhmm.h,
include/mgx_sortdedup.h, include/mgx_smithwaterman.h, include/mgx_realign.h, include/mgx_activity.h, include/mgx_bgzf.h, include/mgx_bam.h, include/mgx_sam.h); there is no Python or CPU compute path.  If the HIP library has not
been built, or no HIP device is visible, every entry point raises.
"""
from . import native  # noqa: F401
from .native import MgxError, lib_path, load  # noqa: F401
from .pairhmm import PairHMMEngine, PairHMMBatch, PairHMMQueue  # noqa: F401
from .sortdedup import SortDedupEngine, Routed  # noqa: F401
from .smithwaterman import SmithWatermanEngine  # noqa: F401
from .realign import RealignEngine  # noqa: F401
from .activity import ActivityEngine  # noqa: F401
from .bgzf import BgzfCompressor, BgzfBatch, BgzfStore, BgzfInflater  # noqa: F401
from .bam import BamScanner  # noqa: F401
from .sam import SamEncoder, lines_host, encode_rules, encode_host  # noqa: F401
from . import pairhmm, sortdedup, smithwaterman, realign, activity, bgzf, bam, sam, synth  # noqa: F401
