// pnc_dense.hip — the host side of the dense PN-Counter merge, A = max(A, B) over identity rows (PNCounter.Merge,
// PNCounters.cs:131-144): the launches of pnc_dense_kernels.hpp's kernels, an int64 store's 32-bit shadow and its state
// (jg::DenseShadow, jg::pnc_merge_dense), and the received batch (jg_rows) in its two forms.  pnc.hip holds the store.
//
// The kernels and their roofline (HBM):
//   k_merge_dense    reads A.P A.N B.P B.N: 4 x elem_bytes per cell (32 B at int64), and writes back only the 128-B
//                    lines of A.P / A.N that a cell of B raised: up to 2 x elem_bytes more (48 B per cell when every
//                    line changes, 32 B for a re-delivered batch).  Two halves of one grid: P's workgroups, then N's
//                    (two read streams at a time); kDenseVecs 16-B vectors of A and of B per lane, non-temporal.
//   k_merge_filtered the same merge of an int64 store by its 32-bit shadow sP / sN = clamp32(P / N): reads sA.P sA.N
//                    B.P B.N, 24 B per cell, and A itself only for lines that hold a cell at a clamp value; writes the
//                    raised lines of A with their 64 B of shadow.  From the third consecutive dense identity merge on
//                    (pnc_merge_dense; k_merge_build writes the shadow at the second); every other writer of P / N
//                    takes them through jg_pnc::rw_P / rw_N, which invalidates the shadow.
//   the narrow form  an int64 identity batch (jg_rows) whose every cell is ABSENT or fits 32 bits is held as 4-byte
//                    codes (pnc_filter.hpp `narrow`) in the lower half of P_ / N_, decided where the batch is born:
//                    jg_rows_upload narrows each landed chunk under the next chunk's copy (k_rows_narrow),
//                    jg_synth_pnc_rows writes the codes.  The three dense kernels read it in place and widen in
//                    registers (k_merge_dense_narrow, k_merge_build / k_merge_filtered with BT = int): a steady launch
//                    reads sA and B at 4 B each, 16 B per cell (P and N), the first launch and the build launch 8 B
//                    less per cell than with a wide batch.  Every other reader goes through jg::rows_wide, which
//                    widens the batch in place first.
#include <algorithm>

#include "launch.hpp"
#include "pnc_dense_kernels.hpp"

namespace {
using namespace jg::filt;

// The two-halves grid of a merge over n_cells cells per array (layout.hpp), refused if it exceeds one launch.
jg::Halves halves(uint64_t n_cells, uint32_t cells_per_unit, uint64_t units_per_block) {
    const jg::Halves h = jg::halves_of(n_cells, cells_per_unit, units_per_block);
    JG_REQUIRE(h.fits(), JG_EINVAL, "merge: %llu cells exceed one launch", (unsigned long long)n_cells);
    return h;
}

// narrow: B is an int64 batch's 4-byte codes (eb == 8 only).
void launch_merge_dense(jg_ctx* ctx, uint32_t eb, void* AP, void* AN, const void* BP, const void* BN, uint64_t n_cells, bool narrow) {
    const jg::Halves h = halves(n_cells, 16 / eb, (uint64_t)kDenseVecs * kDenseBlock);  // units: 16-B vectors
    const unsigned half = (unsigned)h.blocks;
    if (narrow) {
        hipLaunchKernelGGL(k_merge_dense_narrow, dim3(2 * half), dim3(kDenseBlock), 0, ctx->stream, (uint4*)AP, (uint4*)AN, (const uint2*)BP,
                           (const uint2*)BN, h.n_units, h.tail, half);
    } else {
        jg::dispatch_eb(eb, [&](auto EB) {
            hipLaunchKernelGGL(k_merge_dense<EB()>, dim3(2 * half), dim3(kDenseBlock), 0, ctx->stream, (uint4*)AP, (uint4*)AN, (const uint4*)BP,
                               (const uint4*)BN, h.n_units, h.tail, half);
        });
    }
    JG_HIP(hipGetLastError());
}

template <int CELLS, int VECS, int BLOCK, class BT>
void launch_merge_filtered(jg_pnc* p, const void* BP, const void* BN, uint64_t n_cells) {
    const jg::Halves h = halves(n_cells, CELLS, (uint64_t)VECS * BLOCK);
    const unsigned half = (unsigned)h.blocks;
    hipLaunchKernelGGL((k_merge_filtered<CELLS, VECS, BLOCK, BT>), dim3(2 * half), dim3(BLOCK), 0, p->ctx->stream, p->P_.as<long long>(),
                       p->N_.as<long long>(), p->shadow.sP.as<int>(), p->shadow.sN.as<int>(), (const BT*)BP, (const BT*)BN, h.n_units, h.tail, half);
    JG_HIP(hipGetLastError());
}

template <class BT> void launch_build_as(jg_pnc* p, const void* BP, const void* BN, const jg::Halves& h) {
    const unsigned half = (unsigned)h.blocks;
    hipLaunchKernelGGL((k_merge_build<kBuildBlock, BT>), dim3(2 * half), dim3(kBuildBlock), 0, p->ctx->stream, p->P_.as<long long>(),
                       p->N_.as<long long>(), p->shadow.sP.as<int>(), p->shadow.sN.as<int>(), (const BT*)BP, (const BT*)BN, h.n_units, h.tail, half);
}

// The build launch over the batch's cells, then the clamp pass over the store's cells behind the batch.
void launch_merge_build(jg_pnc* p, const void* BP, const void* BN, uint64_t n_cells, bool narrow) {
    const jg::Halves h = halves(n_cells, 2, kBuildBlock);
    if (narrow) launch_build_as<int>(p, BP, BN, h);
    else launch_build_as<long long>(p, BP, BN, h);
    const uint64_t all = p->n_keys * p->R;
    if (n_cells < all) {
        const unsigned g = jg::grid_for(p->ctx, all - n_cells, 256, 16);
        hipLaunchKernelGGL(k_shadow_clamp, dim3(g), dim3(256), 0, p->ctx->stream, p->P_.as<long long>(), p->shadow.sP.as<int>(), n_cells, all);
        hipLaunchKernelGGL(k_shadow_clamp, dim3(g), dim3(256), 0, p->ctx->stream, p->N_.as<long long>(), p->shadow.sN.as<int>(), n_cells, all);
    }
    JG_HIP(hipGetLastError());
}

// ---- the narrow form of a received batch (above; jg_rows in jg_internal.hpp, pnc_filter.hpp) ---------
constexpr size_t kNarrowFlagAt = 128;  // the upload's "a cell does not fit" word in ctx->flags (zero between calls)
// Cells per staged chunk of an upload: at most a quarter of an array (two chunks fit the free upper half), capped at
// 128 MB: every chunk costs the link a launch's worth of host time, and only the last chunk's narrowing (about 50 us
// at the cap) is not hidden under a copy.
constexpr uint64_t kNarrowChunkCap = 16777216;

// One array widened in place, back to front by halves: the pass over cells [ceil(hi / 2), hi) writes only bytes no
// code of a later pass lies in; a batch of n cells takes log2(n / kRowsBlock) launches (this path is correct, not fast).
void widen_in_place(jg_ctx* ctx, void* buf, uint64_t n_cells) {
    uint64_t hi = n_cells;
    while (hi > (uint64_t)kRowsBlock) {
        const uint64_t lo = (hi + 1) / 2;
        hipLaunchKernelGGL(k_rows_widen, dim3(jg::grid_for(ctx, hi - lo, kRowsBlock, 16)), dim3(kRowsBlock), 0, ctx->stream, buf, lo, hi);
        hi = lo;
    }
    hipLaunchKernelGGL(k_rows_widen_small, dim3(1), dim3(kRowsBlock), 0, ctx->stream, buf, (uint32_t)hi);
    JG_HIP(hipGetLastError());
}

// One host array of n int64 cells into `buf` (8 n bytes) as codes.  Chunk k is copied into staging slot k & 1 of the
// upper half and narrowed into the lower half on one and the same stream, and the chunks alternate between ctx->stream
// and ctx->copy (`turn` runs on across P and N): a chunk's narrowing runs under the next chunk's copy, a slot's next
// copy is ordered behind the kernel that reads it by its stream alone, and between two copies the host issues nothing
// but one launch (a copy from pageable memory holds the host, so every call between two of them idles the link).
void upload_narrow_array(jg_ctx* ctx, unsigned& turn, void* buf, const void* host, uint64_t n) {
    auto* flag = reinterpret_cast<unsigned*>(ctx->flags.as<char>() + kNarrowFlagAt);
    const uint64_t stage_at = jg::round_up(n * 4, 16);                      // behind the codes, vector-aligned
    const uint64_t room = n * 8 > stage_at ? n * 8 - stage_at : 0;          // n = 1: the aligned end lies past the buffer
    const uint64_t chunk = std::min<uint64_t>(room / 16, kNarrowChunkCap);  // two slots of `chunk` cells
    if (chunk == 0) {  // n <= 3: no room to stage
        JG_HIP(hipMemcpyAsync(buf, host, n * 8, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_rows_narrow_small, dim3(1), dim3(kRowsBlock), 0, ctx->stream, buf, (uint32_t)n, flag);
        JG_HIP(hipGetLastError());
        return;
    }
    char* const stage = static_cast<char*>(buf) + stage_at;
    uint64_t k = 0;
    for (uint64_t c0 = 0; c0 < n; c0 += chunk, ++k, ++turn) {
        const uint64_t len = std::min(chunk, n - c0);
        hipStream_t st = (turn & 1) ? ctx->copy : ctx->stream;
        long long* const dst = reinterpret_cast<long long*>(stage + (k & 1) * chunk * 8);
        JG_HIP(hipMemcpyAsync(dst, static_cast<const char*>(host) + c0 * 8, len * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_rows_narrow, dim3(jg::grid_for(ctx, len, kRowsBlock, 8)), dim3(kRowsBlock), 0, st, dst, static_cast<int*>(buf) + c0, len,
                           flag);
    }
    JG_HIP(hipGetLastError());
}

// jg_rows_upload of an int64 identity batch with narrowing on.  true: every cell fitted and the batch holds its codes;
// false: a cell did not fit (the buffers hold partial codes: the caller uploads wide).  Both streams have drained.
bool upload_narrow(jg_rows* r, const void* P, const void* N) {
    jg_ctx* ctx = r->ctx;
    const uint64_t n = r->n_rows * r->R;
    JG_HIP(hipStreamSynchronize(ctx->stream));  // an asynchronous merge may still read the buffers ctx->copy is about to write
    unsigned turn = 0;
    upload_narrow_array(ctx, turn, r->P_.p, P, n);
    upload_narrow_array(ctx, turn, r->N_.p, N, n);
    JG_HIP(hipStreamSynchronize(ctx->copy));
    jg::pin_get(ctx, 0, ctx->flags.as<char>() + kNarrowFlagAt, sizeof(unsigned));
    jg::pin_sync(ctx);
    if (*static_cast<const unsigned*>(jg::pin_at(ctx, 0)) == 0) return true;
    JG_HIP(hipMemsetAsync(ctx->flags.as<char>() + kNarrowFlagAt, 0, sizeof(unsigned), ctx->stream));
    return false;
}

}  // namespace

// ---- the shadow ------------------------------------------------------------------------------------------------------
// The buffers are kept across cold spells.  A failed allocation is remembered until the shape changes (drop), so a
// store that does not fit does not ask the allocator on every merge.
bool jg::DenseShadow::ready(size_t bytes) {
    if (sP.p && sN.p && sP.bytes >= bytes && sN.bytes >= bytes) return true;
    if (nomem) return false;
    try {
        sP.alloc(bytes);
        sN.alloc(bytes);
    } catch (const jg::Error&) {
        sP.release();
        sN.release();
        nomem = true;
        (void)hipGetLastError();  // the failed allocation's code must not surface at the next launch check
        jg::clear_error();
        return false;
    }
    return true;
}

void jg::DenseShadow::drop() {
    sP.release();
    sN.release();
    state_ = kCold;
    nomem = false;
}

// int32 stores and stores with the filter off run k_merge_dense and stay cold.  An int64 store runs it while cold (and
// becomes armed: nothing else has written since this merge), the build launch while armed (and becomes valid), the
// filtered kernel while valid.  Every one of the three kernels reads a narrow batch as 4-byte codes.
void jg::pnc_merge_dense(jg_pnc* p, const void* BP, const void* BN, uint64_t n_rows, bool narrow) {
    jg_ctx* ctx = p->ctx;
    DenseShadow& sh = p->shadow;
    const uint64_t n_cells = n_rows * p->R;
    if (p->eb == 8 && sh.on) {
        if (sh.state_ == DenseShadow::kValid)
            return narrow ? launch_merge_filtered<kNarrowCells, kNarrowVecs, kNarrowBlock, int>(p, BP, BN, n_cells)
                          : launch_merge_filtered<kFiltCells, kFiltVecs, kFiltBlock, long long>(p, BP, BN, n_cells);
        if (sh.state_ == DenseShadow::kArmed && sh.ready((size_t)p->n_keys * p->R * 4)) {
            launch_merge_build(p, BP, BN, n_cells, narrow);
            sh.state_ = DenseShadow::kValid;
            return;
        }
        launch_merge_dense(ctx, 8, p->P_.p, p->N_.p, BP, BN, n_cells, narrow);
        sh.state_ = DenseShadow::kArmed;
        return;
    }
    launch_merge_dense(ctx, p->eb, p->rw_P(), p->rw_N(), BP, BN, n_cells, narrow);
}

jg::WideRows jg::rows_wide(const jg_rows* r) {
    if (r->narrow) {
        const uint64_t n = r->n_rows * r->R;
        widen_in_place(r->ctx, r->P_.p, n);
        widen_in_place(r->ctx, r->N_.p, n);
        r->narrow = false;
    }
    return WideRows{r->P_.p, r->N_.p};
}

extern "C" {

int jg_pnc_set_dense_filter(jg_pnc* p, int on) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::check_store(p, "jg_pnc_set_dense_filter");
        p->shadow.on = on != 0;
        if (!p->shadow.on) {
            jg::ensure_device(p->ctx);
            JG_HIP(hipStreamSynchronize(p->ctx->stream));  // an asynchronous merge may still read the shadow
            p->shadow.drop();
        }
    });
}

int jg_pnc_dense_filter_state(jg_pnc* p, int* state) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::check_store(p, "jg_pnc_dense_filter_state");
        JG_REQUIRE(state, JG_EINVAL, "jg_pnc_dense_filter_state: NULL output");
        *state = p->shadow.on ? p->shadow.state() : 0;
    });
}

int jg_rows_create(jg_ctx* ctx, uint64_t n_rows, uint32_t n_replicas, uint32_t elem_bytes, jg_rows** out) {
    return jg::guard([&] {
        auto lk_ = jg::lock(ctx);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(ctx && out, JG_EINVAL, "jg_rows_create: NULL argument");
        JG_REQUIRE(elem_bytes == 4 || elem_bytes == 8, JG_EINVAL, "jg_rows_create: elem_bytes must be 4 or 8");
        JG_REQUIRE(n_rows > 0 && n_replicas > 0, JG_EINVAL, "jg_rows_create: empty shape");
        jg::ensure_device(ctx);
        auto* r = new jg_rows();
        r->ctx = ctx; r->n_rows = n_rows; r->R = n_replicas; r->eb = elem_bytes;
        try {
            const size_t bytes = (size_t)n_rows * n_replicas * elem_bytes;
            r->P_.alloc(bytes);
            r->N_.alloc(bytes);
        } catch (...) {
            delete r;
            throw;
        }
        *out = r;
    });
}

int jg_rows_destroy(jg_rows* r) {
    return jg::guard([&] {
        auto lk_ = jg::lock(r);  // calls on one context are serialised (shared scratch, stream)
        if (!r) return;
        jg::ensure_device(r->ctx);
        JG_HIP(hipStreamSynchronize(r->ctx->stream));
        delete r;
    });
}

int jg_rows_upload(jg_rows* r, const uint32_t* key_idx, const void* P, const void* N) {
    return jg::guard([&] {
        auto lk_ = jg::lock(r);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(r && P && N, JG_EINVAL, "jg_rows_upload: NULL argument");
        jg_ctx* ctx = r->ctx;
        jg::ensure_device(ctx);
        const size_t bytes = (size_t)r->n_rows * r->R * r->eb;
        r->narrow = false;
        // an int64 identity batch is narrowed chunk by chunk as it lands; one that holds a cell that does not fit is
        // copied again, wide (rare: correct, not fast), as every keyed and every int32 batch is in the first place
        if (!key_idx && r->eb == 8 && r->narrow_on) r->narrow = upload_narrow(r, P, N);
        if (!r->narrow) {
            JG_HIP(hipMemcpyAsync(r->P_.p, P, bytes, hipMemcpyHostToDevice, ctx->stream));
            JG_HIP(hipMemcpyAsync(r->N_.p, N, bytes, hipMemcpyHostToDevice, ctx->stream));
        }
        if (key_idx) {
            uint32_t mx = 0;
            for (uint64_t i = 0; i < r->n_rows; ++i) mx = key_idx[i] > mx ? key_idx[i] : mx;
            r->max_key = mx;
            if (r->keys.bytes < r->n_rows * 4) r->keys.alloc(r->n_rows * 4);
            JG_HIP(hipMemcpyAsync(r->keys.p, key_idx, r->n_rows * 4, hipMemcpyHostToDevice, ctx->stream));
            r->has_keys = true;
        } else {
            r->has_keys = false;
        }
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int jg_pnc_merge_batch(jg_pnc* p, const jg_rows* r, int async) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_merge_batch");
        jg::check_store(p, "jg_pnc_merge_batch");
        JG_REQUIRE(r, JG_EINVAL, "jg_pnc_merge_batch: rows is NULL");
        JG_REQUIRE(r->ctx == p->ctx, JG_EINVAL, "jg_pnc_merge_batch: rows and store belong to different contexts");
        JG_REQUIRE(r->R == p->R && r->eb == p->eb, JG_ETYPE, "jg_pnc_merge_batch: row shape (%u x %uB) != store (%u x %uB)", r->R, r->eb,
                   p->R, p->eb);
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        if (r->has_keys) {
            JG_REQUIRE(r->max_key < p->n_keys, JG_EINVAL, "jg_pnc_merge_batch: batch addresses key %u >= n_keys %llu", r->max_key,
                       (unsigned long long)p->n_keys);
            const jg::WideRows w = jg::rows_wide(r);  // a keyed batch is wide already
            jg::pnc_merge_indexed(p, w.P, w.N, r->keys.as<uint32_t>(), r->n_rows);
        } else {
            JG_REQUIRE(r->n_rows <= p->n_keys, JG_EINVAL, "jg_pnc_merge_batch: identity batch of %llu rows > n_keys",
                       (unsigned long long)r->n_rows);
            jg::pnc_merge_dense(p, r->P_.p, r->N_.p, r->n_rows, r->narrow);  // the one reader of either form in place
        }
        if (!async) JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int jg_rows_set_narrow(jg_rows* r, int on) {
    return jg::guard([&] {
        auto lk_ = jg::lock(r);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(r, JG_EINVAL, "jg_rows_set_narrow: rows is NULL");
        r->narrow_on = on != 0;
        if (!r->narrow_on && r->narrow) {
            jg::ensure_device(r->ctx);
            jg::rows_wide(r);
            JG_HIP(hipStreamSynchronize(r->ctx->stream));
        }
    });
}

int jg_rows_form(jg_rows* r, int* form) {
    return jg::guard([&] {
        auto lk_ = jg::lock(r);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(r && form, JG_EINVAL, "jg_rows_form: NULL argument");
        *form = r->narrow ? 1 : 0;
    });
}

}  // extern "C"
