// The engine's work-space arena (cp_model::arena) and the scope guard of one allocation.  Plain C++ with no HIP include, so that
// the host compiler can build it too (tests/native/arena_host.cpp, tests/test_arena_cpu.py checks it against a brute-force
// interval model).
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace cp_engine {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---------------------------------------------------------------------------------------------
// Deterministic first-fit arena over a caller-provided workspace.  A dry run (base == nullptr)
// replays the same allocation sequence to measure the peak, so cp_model_workspace_bytes() and
// cp_model_forward() always agree.
// alloc never fails: a block that ends beyond `cap` gets its offset all the same and sets `overflow`.  Nothing may be
// launched on such an offset unchecked: the entry points compare the caller's size with the query before the first launch
// (engine.hip: workspace_refused), and `overflow` after the pass is the backstop behind that.
// ---------------------------------------------------------------------------------------------
struct Arena {
    char* base = nullptr;
    size_t cap = 0, peak = 0;
    bool overflow = false;
    std::vector<std::pair<size_t, size_t>> free_;  // (offset, size), sorted by offset

    void reset(void* b, size_t c) {
        base = (char*)b;
        cap = c;
        peak = 0;
        overflow = false;
        free_.clear();
        free_.push_back({0, (size_t)1 << 62});
    }
    size_t alloc(size_t bytes) {
        bytes = align_up(bytes, 256);
        for (size_t i = 0; i < free_.size(); ++i) {
            if (free_[i].second >= bytes) {
                const size_t off = free_[i].first;
                free_[i].first += bytes;
                free_[i].second -= bytes;
                if (free_[i].second == 0) free_.erase(free_.begin() + i);
                if (off + bytes > peak) peak = off + bytes;
                if (base && off + bytes > cap) overflow = true;
                return off;
            }
        }
        overflow = true;
        return 0;
    }
    void release(size_t off, size_t bytes) {
        bytes = align_up(bytes, 256);
        size_t i = 0;
        while (i < free_.size() && free_[i].first < off) ++i;
        free_.insert(free_.begin() + i, {off, bytes});
        if (i + 1 < free_.size() && free_[i].first + free_[i].second == free_[i + 1].first) {
            free_[i].second += free_[i + 1].second;
            free_.erase(free_.begin() + i + 1);
        }
        if (i > 0 && free_[i - 1].first + free_[i - 1].second == free_[i].first) {
            free_[i - 1].second += free_[i].second;
            free_.erase(free_.begin() + i);
        }
    }
};

struct Block {
    Arena* a;
    size_t off, bytes;
    Block(Arena* a_, size_t b) : a(a_), off(a_->alloc(b)), bytes(b) {}
    ~Block() { a->release(off, bytes); }
};

}  // namespace cp_engine
