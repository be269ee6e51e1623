// The 64-bit rolling hash shared by the device beam search (ctc_beam.hip: prefix hashes, partial-word hashes, LM table
// keys) and the host that builds the LM tables (codes/lm.py: seq_hash, the same function in Python).  Plain C++ as well:
// tests/test_lm_cpu.py compiles a two-line host program against this header to check that both sides agree.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define DS2_HD __host__ __device__
#else
#define DS2_HD
#endif

#define DS2_HASH_SEED 0x243F6A8885A308D3ull
#define DS2_HASH_STEP 0x9E3779B97F4A7C15ull

// splitmix64's finaliser
DS2_HD inline uint64_t ds2_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// one step: the hash of a sequence extended by the id x
DS2_HD inline uint64_t ds2_hash_step(uint64_t h, int x) { return ds2_mix64(h + DS2_HASH_STEP + (uint64_t)(uint32_t)x); }
// a table key: never 0 (0 marks an empty slot)
DS2_HD inline uint64_t ds2_hash_key(uint64_t h) { return h ? h : 1; }
