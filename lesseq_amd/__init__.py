"""lesseq_amd -- MI355X-native count + solve path of LESSeq.

The product is the C-ABI library `liblesseq_hip.so` (include/lesseq_hip.h: host logic in C++,
hand-written HIP kernels for gfx950) and the `count` / `solve` / `classify` / `test_as` / `events` / `parseGencode` / `gencodeIsoformMap` / `sam2mrf` / `bam2mrf` / `bamcheck` / `junctions` / `coverage` / `exonbins` / `psi` / `evidence` / `sites` / `retention` / `clusters` / `libtype` executables built
from it.  This package is only the ctypes binding used by the tests and bench.py; it holds
no compute of its own and refuses to import without the built library.
"""
from ._lib import lib, LsqError, check  # noqa: F401
from .api import (Annotation, Events, Reads, Context, SynthSpec, cli_run, synth_write, synth_write_sam,  # noqa: F401
                  format_count, format_solve, EVENT_TYPES, sam_to_mrf, bam_to_mrf, bam_check_host, SAM_DEFAULT_SKIP_FLAGS,
                  bootstrap_resample_host, bootstrap_draws)
from .diffsplice import fisher, lrt, wilcox, adjust, betabin  # noqa: F401
from . import localevents  # noqa: F401
from . import gencode  # noqa: F401
from .gencode import parse_gtf, isoform_map  # noqa: F401
from . import junctions  # noqa: F401
from .junctions import JunctionIndex  # noqa: F401
from . import coverage  # noqa: F401
from .coverage import CoverageIndex  # noqa: F401
from . import exonbins  # noqa: F401
from .exonbins import ExonBinIndex, ExonBins  # noqa: F401
from . import libtype  # noqa: F401
from .libtype import LibTypeIndex, LibType  # noqa: F401
from . import psi  # noqa: F401
from .psi import PsiIndex, Psi  # noqa: F401
from . import evidence  # noqa: F401
from .evidence import EvidenceIndex, Evidence  # noqa: F401
from . import sites  # noqa: F401
from .sites import SiteIndex, Sites  # noqa: F401
from . import retention  # noqa: F401
from .retention import RetentionIndex, Retention  # noqa: F401
from . import clusters  # noqa: F401
from .clusters import ClusterPool, Clusters  # noqa: F401

__all__ = ["lib", "LsqError", "check", "Annotation", "Events", "Reads", "Context", "SynthSpec",
           "cli_run", "synth_write", "synth_write_sam", "sam_to_mrf", "bam_to_mrf", "bam_check_host", "SAM_DEFAULT_SKIP_FLAGS", "format_count", "format_solve", "EVENT_TYPES",
           "fisher", "lrt", "wilcox", "adjust", "betabin", "localevents", "gencode", "parse_gtf", "isoform_map", "junctions", "JunctionIndex", "coverage", "CoverageIndex", "exonbins", "ExonBinIndex", "ExonBins", "libtype", "LibTypeIndex", "LibType", "psi", "PsiIndex", "Psi", "evidence", "EvidenceIndex", "Evidence", "sites", "SiteIndex", "Sites", "retention", "RetentionIndex", "Retention", "clusters", "ClusterPool", "Clusters", "bootstrap_resample_host", "bootstrap_draws"]
