// engine_graph.h -- the graph caches of libpgmi's host side, and the contract that makes a replay the call.
//
// A context holds two caches (pgmi_ctx::pgraphs: vision tower and language-model forward; pgmi_ctx::dgraphs: decode
// steps).  run_graphed replays a captured hipGraph when a call's key is one it has captured, so the launches of
// that call are the launches of an earlier one.  That is the eager call only while the following holds.
//
// 1. The key holds every pointer and size the body passes to a launch: the caller's buffers, the batch and
//    sequence sizes, the flags that choose a kernel form, and (prefill) the tuning epoch, which every pgmi_tune_*
//    call bumps -- a forced GEMM plan or attention variant changes which kernels a body launches.  The keys are
//    built here alone (prefill_key, decode_key).
//
// 2. Besides the key a body reads only
//      - the config (pgmi_ctx::c), fixed at pgmi_create;
//      - buffers allocated once, by the first pgmi_prepare (Hs ... lm_done, cosT / sinT, patch_w, ws): their
//        addresses never change, their contents are read at run time;
//      - the launch state below, whose every writer calls graphs_drop for the graphs that read it.
//    A body takes `const pgmi_ctx*` (vision_body, lm_entry, lm_body, lm_rows and the lm_* stages, decode_head /
//    layer / tail / body): it cannot change host state that a replay would not repeat.
//
// 3. The launch state and its writers (what each drops):
//      w (slab pointers)         bind_tables <- pgmi_bind_weights                         all
//      w.t[i].mf_*, mfw          ensure_mf_image, when it allocates the images            decode, small and batched
//                                (a rebuild after pgmi_prepare / pgmi_lora_set is in place: same pointers)
//      (the 13-bit images, per form f; pk_graphs(f): rows -> decode B <= 2, prefill; fragment -> decode B >= 3)
//      w.t[i].pk_*[f],           ensure_pk_image, when it changed pk[f].done              pk_graphs(f)
//      w.pk_embed[f], pk[f].done pk_forget <- pgmi_bind_weights, pgmi_prepare             all
//                                pk_forget_kinds <- pgmi_lora_set (gate / up / down)      pk_graphs(f), where f had one done
//      pk[f].mask                pgmi_set_decode_packed (rows) / _batched (fragment)      pk_graphs(f)
//      mf_staged                 pgmi_set_decode_staged_norm                              decode, small and batched
//      probe_on, probe_ev        pgmi_prefill_probe (prefill graphs are off while on)     prefill
//      prefill_graph             pgmi_set_prefill_graph, pgmi_prefill_probe               prefill
//      everything                pgmi_prepare, pgmi_destroy                               all
//    The prefill reads the 13-bit images too: a last-row-only prefill (logits_rows 2) and every lm_head over last
//    rows run the decode GEMVs, which pk_use switches by the row form's mask and done (never the fragment form's).
//
// 4. What each call rewrites outside the graph, before it: the positions (dpos, lm_begin), a ragged prefill's row
//    lengths (d_rlens, lm_begin), the step records (step / rstep: set when the call does not continue the last
//    one, advanced by the step's last kernel inside the graph), and the staged inputs of a graphed decode step
//    (d_ids, d_emb, d_mask).  A prefix-LM prefill (pgmi_lm_forward_prefix) rewrites its rows' key counts and prefix
//    lengths (d_rlens segments 2 and 3) the same way, and then has no graph at all: it runs its body on the caller's
//    stream, and neither looks up nor inserts a key in pgraphs (the per-query key limits of k_attn_fs are not a
//    replayed form; a scoring call's buffers are fresh each time).  The host mirrors (tn_rows, step_known and its
//    fellows) are written around the body, never in it.
//
// 5. Non-kernel nodes: a prefill graph holds three kinds, per row group -- the memset of pstep->kv_len and the 2-D
//    copy into lastrows of lm_last_row_tail (logits_rows 2), or the 2-D copy into lastrows of lm_logits
//    (logits_rows 1, lock-step).  A decode graph holds none.
//
// 6. Eager first: the first call with a key runs its body on the caller's stream, the second captures it.  The
//    launchers set kernel attributes on a kernel's first launch (their `static attr` pattern), and that is no
//    stream operation: it must not happen first inside a capture.  So a body is captured only after the very
//    launches it makes have run eagerly once, which is why a change of launch state drops the keys that were merely
//    seen (null entries) together with the captured ones.
//
// Entries are erased here and nowhere else: graphs_drop, the size bound in run_graphed, and the failure path's
// erase of its own key.
#pragma once
#include "engine_ctx.h"

inline void GraphCache::clear() {
    for (auto& kv : map)
        if (kv.second) (void)hipGraphExecDestroy(kv.second);
    map.clear();
}

namespace pgmi_eng __attribute__((visibility("hidden"))) {

// what graphs_drop drops: the prefill graphs, the captured decode steps of B <= 2 rows (the streaming GEMVs, which
// read the 13-bit images), those of more rows
enum { GRAPHS_PREFILL = 1, GRAPHS_DECODE_SMALL = 2, GRAPHS_DECODE_BATCHED = 4,
       GRAPHS_DECODE = GRAPHS_DECODE_SMALL | GRAPHS_DECODE_BATCHED, GRAPHS_ALL = GRAPHS_PREFILL | GRAPHS_DECODE };

// the graphs whose launches hold a form's 13-bit images (or their absence): the B <= 2 steps and the prefill's
// last-row GEMVs read the row form, the batched steps the fragment form
inline int pk_graphs(PkForm f) { return f == PK_FORM_FRAG ? GRAPHS_DECODE_BATCHED : GRAPHS_DECODE_SMALL | GRAPHS_PREFILL; }

// A prefill key: the kind of call (1 vision tower, 2 language-model forward), its arguments, the tuning epoch.
inline std::vector<intptr_t> prefill_key(int kind, std::initializer_list<intptr_t> args) {
    std::vector<intptr_t> key{kind};
    key.insert(key.end(), args.begin(), args.end());
    key.push_back((intptr_t)tune_epoch());
    return key;
}

// A decode key: the batch first (graphs_drop tells the B <= 2 steps from the batched ones by it), then the rest.
inline std::vector<intptr_t> decode_key(int B, std::initializer_list<intptr_t> rest) {
    std::vector<intptr_t> key{B};
    key.insert(key.end(), rest.begin(), rest.end());
    return key;
}

// The one invalidation: the caller names what its change of launch state invalidates (the table above).
inline void graphs_drop(pgmi_ctx* x, int what) {
    if (what & GRAPHS_PREFILL) x->pgraphs.clear();
    if ((what & GRAPHS_DECODE) == GRAPHS_DECODE) {
        x->dgraphs.clear();
        return;
    }
    auto& m = x->dgraphs.map;
    for (auto it = m.begin(); it != m.end();) {
        const bool small = !it->first.empty() && it->first[0] <= 2;  // decode_key: key[0] = B
        if (what & (small ? GRAPHS_DECODE_SMALL : GRAPHS_DECODE_BATCHED)) {
            if (it->second) (void)hipGraphExecDestroy(it->second);
            it = m.erase(it);
        } else {
            ++it;
        }
    }
}

// The one graph policy: the first call with a key runs body(s) eagerly (kernel attributes are set on first launch),
// the second captures body(cap_stream), instantiates and launches, later ones replay.  A key that would be entry
// PGMI_GRAPH_CACHE_MAX + 1 drops the whole cache first (fresh buffers every call must not grow it without bound).
// sync_before_capture: the decode step's hipStreamSynchronize(s); the prefill has none (pgmi_vision may be called
// where a synchronise is not allowed).
template <class F>
int run_graphed(pgmi_ctx* x, GraphCache& gc, hipStream_t s, const std::vector<intptr_t>& key, F body,
                bool sync_before_capture) {
    auto it = gc.map.find(key);
    if (it == gc.map.end()) {
        if (gc.map.size() >= PGMI_GRAPH_CACHE_MAX) gc.clear();
        gc.map[key] = nullptr;
        return body(s);
    }
    if (it->second) {
        HIPCHK(hipGraphLaunch(it->second, s));
        return 0;
    }
    // Capture.  Whatever fails from here on: an opened capture is ended, a graph we got is destroyed and the key's
    // entry is erased (the next call with it starts over, eagerly); the first error is the one reported.
    hipGraph_t g = nullptr;
    hipGraphExec_t exec = nullptr;
    int rc = 0;
    hipError_t e = sync_before_capture ? hipStreamSynchronize(s) : hipSuccess;
    if (e == hipSuccess && (e = hipStreamBeginCapture(x->cap_stream, hipStreamCaptureModeThreadLocal)) == hipSuccess) {
        rc = body(x->cap_stream);  // may fail and return (HIPCHK) with the capture open: it is ended here
        const hipError_t end = hipStreamEndCapture(x->cap_stream, &g);
        if (rc == 0) e = end;
    }
    if (rc == 0 && e == hipSuccess) e = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    if (g) (void)hipGraphDestroy(g);
    if (rc == 0 && e == hipSuccess) e = hipGraphLaunch(exec, s);
    if (rc == 0 && e == hipSuccess) {
        gc.map[key] = exec;
        return 0;
    }
    if (exec) (void)hipGraphExecDestroy(exec);
    gc.map.erase(key);
    return rc ? rc : fail(PGMI_E_HIP, std::string("hipGraph capture: ") + hipGetErrorString(e));
}

// prefill calls (vision tower, language-model forward): one body, and no graph at all while prefill_graph is off
template <class F>
int run_prefill(pgmi_ctx* x, hipStream_t s, const std::vector<intptr_t>& key, F body) {
    if (!x->prefill_graph) return body(s);
    return run_graphed(x, x->pgraphs, s, key, body, false);
}

}  // namespace pgmi_eng
