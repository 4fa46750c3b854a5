"""Python binding + tooling of the MI355X SMEM seeding engine (libsmemgpu.so)."""
from .lib import (AlnResults, Batch, FinResults, Gpu, Index, SA, Options, Results, SamResults, SmemError, aln_opt, build_id,
                  device_count,
                  fin_opt, kernel_id, load, matesw_opt, pair_opt, pestat_opt, seed, source_hash)  # noqa: F401
