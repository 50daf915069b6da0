"""distpow -- MI355X-native proof-of-work search (philipjesic/Distributed-Proof-Of-Work hot path).

The worker's brute-force search (worker.go:258-401) runs as a hand-written gfx950
HIP kernel in libdpow.so; this package is the host side above its C ABI.
"""
from ._lib import (CANCELLED, DPOW_K_LIMIT, DPOW_MAX_SECRET, DPOW_NO_HIT, EAGAIN, EHIP, EINVAL, EPROTO, ERANGE,
                   EVERIFY, EXHAUSTED, FOUND, LIB_PATH, DpowError, build_id, lib)
from ._lib import MORE, SCAN_DEVICE_MIN_HITS
from .search import scan_device_cut, scan_batch_device_settle, DigestTask, digests_batch_walk
from .search import (BatchTask, Miner, QueueResult, Census, CensusTask, census_plan, ScanHit, ScanTask, scan_plan, scan_plan_halve, SearchResult, TaskQueue, batch_candidate, batch_plan, batch_plan_block, device_count,
                     digest_of_index, global_index, md5, plan_candidate, plan_window, queue_plan,
                     remainder_bits, scan_slice, secret_from_index, thread_bytes, trailing_zero_nibbles, verify)

__all__ = ["Miner", "SearchResult", "BatchTask", "batch_candidate", "batch_plan", "batch_plan_block",
           "TaskQueue", "QueueResult", "queue_plan", "EAGAIN", "ScanHit", "scan_slice", "MORE", "Census",
           "CensusTask", "census_plan", "ScanTask", "scan_plan", "scan_plan_halve",
           "digest_of_index", "DigestTask", "digests_batch_walk", "scan_device_cut", "SCAN_DEVICE_MIN_HITS", "scan_batch_device_settle",
           "DpowError", "lib", "LIB_PATH", "device_count", "md5", "verify",
           "secret_from_index", "trailing_zero_nibbles", "thread_bytes", "remainder_bits", "global_index",
           "plan_window", "plan_candidate", "DPOW_NO_HIT", "DPOW_K_LIMIT", "DPOW_MAX_SECRET", "FOUND",
           "EXHAUSTED", "CANCELLED", "EINVAL", "EHIP", "EVERIFY", "ERANGE", "EPROTO", "build_id"]
