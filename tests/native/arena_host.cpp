// The engine's work-space arena (centerpose_amd/csrc/engine_arena.h) built for the host, driven one operation at a time by
// tests/test_arena_cpu.py.  Blocks are taken and returned through cp_engine::Block, the scope guard the engine's tensors hold.
// A "real" arena gets a base pointer that is never dereferenced (the arena only adds offsets to it); a dry one gets null.
#include "../../centerpose_amd/csrc/engine_arena.h"

#include <map>
#include <memory>

namespace {
struct Host {
    cp_engine::Arena arena;
    std::map<int, std::unique_ptr<cp_engine::Block>> live;
    int next = 0;
};
}  // namespace

extern "C" {

void* arena_host_new(int real, size_t cap) {
    Host* h = new Host;
    h->arena.reset(real ? (void*)0x1000 : nullptr, cap);
    return h;
}

void arena_host_delete(void* p) { delete (Host*)p; }

// -> the block's id; *off: where the arena put it
int arena_host_alloc(void* p, size_t bytes, size_t* off) {
    Host* h = (Host*)p;
    const int id = h->next++;
    h->live[id].reset(new cp_engine::Block(&h->arena, bytes));
    *off = h->live[id]->off;
    return id;
}

void arena_host_release(void* p, int id) { ((Host*)p)->live.erase(id); }

void arena_host_state(void* p, size_t* peak, int* overflow, size_t* cap, int* has_base) {
    Host* h = (Host*)p;
    *peak = h->arena.peak;
    *overflow = h->arena.overflow ? 1 : 0;
    *cap = h->arena.cap;
    *has_base = h->arena.base != nullptr;
}

// the free list as (offset, size) pairs -> how many there are (at most `max` are written)
int arena_host_free_list(void* p, size_t* out, int max) {
    Host* h = (Host*)p;
    int n = 0;
    for (const auto& f : h->arena.free_) {
        if (n < max) {
            out[2 * n] = f.first;
            out[2 * n + 1] = f.second;
        }
        ++n;
    }
    return n;
}

size_t arena_host_align_up(size_t x, size_t a) { return cp_engine::align_up(x, a); }

}  // extern "C"
