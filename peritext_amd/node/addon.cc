/*
 * addon.cc — N-API binding of the C ABI in include/peritext_hip.h (the TypeScript/JS host's door to the GPU).
 *
 * The reference has no FFI: bridge.ts:253/288 and the test harness (test/micromerge.ts:54-79) call
 * Micromerge.applyChange / getTextWithFormatting on JS objects.  This addon is what a maintainer adds instead
 * (INTEGRATION.md): index.js flattens `Change[]` into the SoA op-log columns, this file hands their ArrayBuffers
 * to ptx_apply_materialize and copies the canonical result rows back into typed arrays.  Nothing is computed
 * here; libperitext_hip.so is dlopen()ed at run time, so the addon builds with plain g++ and no ROCm headers:
 *     g++ -O2 -shared -fPIC -I/usr/include/node -Iinclude peritext_amd/node/addon.cc -ldl -o peritext_amd/node/peritext_node.node
 *
 * Exports:  open(libPath) -> abiVersion      create(device, flags) -> ctx (external)      destroy(ctx)
 *           applyMaterialize(ctx, batch) -> {logs:Uint32Array(12/log), values:Uint32Array, spans:Uint32Array(2/row),
 *                                            cintervals:Uint32Array(3/row), valueOff / spanOff / cintOff: BigUint64Array(nLogs + 1) (the rows are compact: ABI 7),
 *                                            elemRank:Uint32Array|null}
 *           generate(ctx, cfg)  change(ctx, batch, inputOps) -> {batch, status}  maxOpsPerLog(ctx)  kernelName()
 * Errors of the library surface as JS exceptions (Error with the library's message); per-LOG failures stay in
 * logs[12*l] (status) and are turned into RangeError by index.js, mirroring micromerge.ts:503,:507,:752.
 */
#include <dlfcn.h>
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/peritext_hip.h"

namespace {

struct Lib {
    void* handle = nullptr;
    uint32_t (*abi_version)(void) = nullptr;
    ptx_status (*create)(int, uint32_t, ptx_ctx**) = nullptr;
    void (*destroy)(ptx_ctx*) = nullptr;
    const char* (*last_error)(const ptx_ctx*) = nullptr;
    ptx_status (*apply_materialize)(ptx_ctx*, const ptx_batch*, ptx_result*) = nullptr;
    void (*result_free)(ptx_result*) = nullptr;
    uint32_t (*max_ops_per_log)(const ptx_ctx*) = nullptr;
    const char* (*kernel_name)(void) = nullptr;
    /* staged form, used when the caller also wants the Patch[] streams */
    ptx_status (*batch_upload)(ptx_ctx*, const ptx_batch*, ptx_dbatch**) = nullptr;
    void (*batch_free)(ptx_ctx*, ptx_dbatch*) = nullptr;
    ptx_status (*result_alloc)(ptx_ctx*, const ptx_dbatch*, ptx_dresult**) = nullptr;
    void (*dresult_free)(ptx_ctx*, ptx_dresult*) = nullptr;
    ptx_status (*merge)(ptx_ctx*, const ptx_dbatch*, ptx_dresult*) = nullptr;
    ptx_status (*sync)(ptx_ctx*) = nullptr;
    ptx_status (*result_download)(ptx_ctx*, const ptx_dbatch*, const ptx_dresult*, ptx_result*) = nullptr;
    ptx_status (*replay_patches)(ptx_ctx*, const ptx_dbatch*, const ptx_dresult*, ptx_patches*) = nullptr;
    /* resident replicas: the logs stay in HBM between calls, new Changes are appended, only their Patch[] records come back */
    ptx_status (*batch_append)(ptx_ctx*, const ptx_dbatch*, const ptx_batch*, ptx_dbatch**) = nullptr;
    ptx_status (*replay_patches_from)(ptx_ctx*, const ptx_dbatch*, const ptx_dresult*, const uint32_t*, ptx_patches*) = nullptr;
    uint32_t (*batch_n_logs)(const ptx_dbatch*) = nullptr;
    void (*patches_free)(ptx_patches*) = nullptr;
    /* on-device change(): op logs generated in HBM */
    ptx_status (*generate)(ptx_ctx*, const ptx_gen_config*, ptx_dbatch**, ptx_gen_info*) = nullptr;
    void (*gen_info_free)(ptx_gen_info*) = nullptr;
    ptx_status (*batch_download)(ptx_ctx*, const ptx_dbatch*, ptx_host_batch*) = nullptr;
    void (*host_batch_free)(ptx_host_batch*) = nullptr;
    /* change(): caller-supplied InputOperations */
    ptx_status (*change)(ptx_ctx*, const ptx_dbatch*, const ptx_dresult*, const ptx_input_ops*, ptx_dbatch**, uint32_t*) = nullptr;
    ptx_status (*batch_append_device)(ptx_ctx*, const ptx_dbatch*, const ptx_dbatch*, ptx_dbatch**) = nullptr;
    /* sync of replica logs: getMissingChanges + applyChanges */
    ptx_status (*sync_replicas)(ptx_ctx*, const ptx_dbatch*, uint32_t, const uint32_t*, const uint32_t*, uint32_t, ptx_dbatch**, uint32_t*) = nullptr;
    /* resident logs at a past version: clock cuts and prefix cuts */
    ptx_status (*batch_at_versions)(ptx_ctx*, const ptx_dbatch*, uint32_t, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, ptx_dbatch**, uint32_t*, uint32_t*, uint32_t*,
                                    uint32_t*) = nullptr;
    /* multi-GPU: the digest all-gather (RCCL inside the library) */
    ptx_status (*comm_unique_id)(ptx_ctx*, uint8_t*) = nullptr;
    ptx_status (*comm_init)(ptx_ctx*, const uint8_t*, uint32_t, uint32_t, ptx_comm**) = nullptr;
    void (*comm_destroy)(ptx_ctx*, ptx_comm*) = nullptr;
    uint32_t (*comm_n_ranks)(const ptx_comm*) = nullptr;
    ptx_status (*allgather_digests)(ptx_ctx*, ptx_comm*, const ptx_dresult*, const uint32_t*, uint64_t*) = nullptr;
    ptx_status (*count_converged_digests)(ptx_ctx*, const uint64_t*, uint64_t, uint32_t, uint64_t*) = nullptr;
    ptx_status (*result_download_logs)(ptx_ctx*, const ptx_dresult*, ptx_log_result*, uint32_t) = nullptr;
    ptx_status (*resolve_cursors)(ptx_ctx*, const ptx_dbatch*, const ptx_dresult*, uint32_t, const uint32_t*, const uint8_t*, const uint64_t*, uint64_t*, uint32_t*) = nullptr;
    /* the map objects of a replica: getRoot() */
    ptx_status (*root_map)(ptx_ctx*, const ptx_dbatch*, ptx_root_maps*) = nullptr;
    void (*root_maps_free)(ptx_root_maps*) = nullptr;
    ptx_status (*device_alloc)(ptx_ctx*, uint64_t, void**) = nullptr;
    void (*device_free)(ptx_ctx*, void*) = nullptr;
    ptx_status (*device_read)(ptx_ctx*, const void*, void*, uint64_t) = nullptr;
    /* patch streams back into canonical rows; the fuzzer's patch assertion on the device */
    ptx_status (*accumulate_patches)(ptx_ctx*, const ptx_dbatch*, const ptx_patches*, ptx_result*) = nullptr;
    ptx_status (*check_patches)(ptx_ctx*, const ptx_dbatch*, const ptx_dresult*, ptx_patch_check_log*, uint64_t*) = nullptr;
    /* document text assembled on the device */
    ptx_status (*strings_upload)(ptx_ctx*, const uint16_t*, const uint64_t*, uint32_t, ptx_dstrings**) = nullptr;
    void (*strings_free)(ptx_ctx*, ptx_dstrings*) = nullptr;
    ptx_status (*result_text_range)(ptx_ctx*, const ptx_dbatch*, const ptx_dresult*, const ptx_dstrings*, uint32_t, uint32_t, ptx_text*) = nullptr;
    void (*text_free)(ptx_text*) = nullptr;
    /* find in that text without downloading it */
    ptx_status (*result_find_text)(ptx_ctx*, const ptx_dbatch*, const ptx_dresult*, const ptx_dstrings*, uint32_t, uint32_t, const uint16_t*, uint32_t, uint32_t, uint32_t, ptx_matches*) = nullptr;
    void (*matches_free)(ptx_matches*) = nullptr;
    /* the text and span rows of element ranges */
    ptx_status (*result_text_slices)(ptx_ctx*, const ptx_dbatch*, const ptx_dresult*, const ptx_dstrings*, uint32_t, uint32_t, const uint64_t*, const uint32_t*, const uint32_t*, ptx_slices*) = nullptr;
    void (*slices_free)(ptx_slices*) = nullptr;
    /* a resident text view: many searches and snippets against one merge */
    ptx_status (*text_view_create)(ptx_ctx*, const ptx_dbatch*, const ptx_dresult*, const ptx_dstrings*, uint32_t, uint32_t, ptx_dview**) = nullptr;
    void (*text_view_free)(ptx_ctx*, ptx_dview*) = nullptr;
    ptx_status (*view_find_text)(ptx_ctx*, const ptx_dview*, const uint16_t*, uint32_t, uint32_t, uint32_t, ptx_matches*) = nullptr;
    ptx_status (*view_text_slices)(ptx_ctx*, const ptx_dview*, const uint64_t*, const uint32_t*, const uint32_t*, ptx_slices*) = nullptr;
    ptx_status (*view_find_snippets)(ptx_ctx*, const ptx_dview*, const uint16_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, ptx_snippets*) = nullptr;
    void (*snippets_free)(ptx_snippets*) = nullptr;
    /* find and replace on a view: hits into change() input */
    ptx_status (*view_replace_plan)(ptx_ctx*, const ptx_dview*, const uint16_t*, uint32_t, uint32_t, const uint32_t*, uint32_t, uint32_t, ptx_replace_plan*) = nullptr;
    void (*replace_plan_free)(ptx_replace_plan*) = nullptr;
    /* a view queried by format: the runs of a mark, their text, a find inside them */
    ptx_status (*view_mark_runs)(ptx_ctx*, const ptx_dview*, uint32_t, uint32_t, uint32_t, ptx_mark_runs*) = nullptr;
    void (*mark_runs_free)(ptx_mark_runs*) = nullptr;
    ptx_status (*view_mark_snippets)(ptx_ctx*, const ptx_dview*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, ptx_mark_snippets*) = nullptr;
    void (*mark_snippets_free)(ptx_mark_snippets*) = nullptr;
    ptx_status (*view_find_in_marks)(ptx_ctx*, const ptx_dview*, const uint16_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, ptx_matches*) = nullptr;
} L;

#define NAPI_OK(call)                                                        \
    do {                                                                     \
        if ((call) != napi_ok) {                                             \
            napi_throw_error(env, nullptr, "N-API call failed: " #call);     \
            return nullptr;                                                  \
        }                                                                    \
    } while (0)

napi_value throw_msg(napi_env env, const char* msg) {
    napi_throw_error(env, nullptr, msg);
    return nullptr;
}

template <class F>
bool sym(F& fn, const char* name) {
    fn = (F)dlsym(L.handle, name);
    return fn != nullptr;
}

napi_value Open(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    char path[4096];
    size_t len = 0;
    if (argc < 1 || napi_get_value_string_utf8(env, argv[0], path, sizeof(path), &len) != napi_ok) return throw_msg(env, "open(libPath): string expected");
    if (!L.handle) {
        L.handle = dlopen(path, RTLD_NOW | RTLD_LOCAL);
        if (!L.handle) {
            char msg[4600];
            snprintf(msg, sizeof(msg), "cannot load %s: %s (build it with __graft_entry__.build(); there is no CPU fallback)", path, dlerror());
            return throw_msg(env, msg);
        }
        bool ok = sym(L.abi_version, "ptx_abi_version") && sym(L.create, "ptx_create") && sym(L.destroy, "ptx_destroy") &&
                  sym(L.last_error, "ptx_last_error") && sym(L.apply_materialize, "ptx_apply_materialize") && sym(L.result_free, "ptx_result_free") &&
                  sym(L.max_ops_per_log, "ptx_max_ops_per_log") && sym(L.kernel_name, "ptx_kernel_name") && sym(L.batch_upload, "ptx_batch_upload") &&
                  sym(L.batch_free, "ptx_batch_free") && sym(L.result_alloc, "ptx_result_alloc") && sym(L.dresult_free, "ptx_dresult_free") &&
                  sym(L.merge, "ptx_merge") && sym(L.sync, "ptx_sync") && sym(L.result_download, "ptx_result_download") &&
                  sym(L.replay_patches, "ptx_replay_patches") && sym(L.batch_append, "ptx_batch_append") && sym(L.replay_patches_from, "ptx_replay_patches_from") &&
                  sym(L.batch_n_logs, "ptx_batch_n_logs") && sym(L.patches_free, "ptx_patches_free") && sym(L.generate, "ptx_generate") &&
                  sym(L.gen_info_free, "ptx_gen_info_free") && sym(L.batch_download, "ptx_batch_download") && sym(L.host_batch_free, "ptx_host_batch_free") && sym(L.change, "ptx_change") &&
                  sym(L.comm_unique_id, "ptx_comm_unique_id") && sym(L.comm_init, "ptx_comm_init") && sym(L.comm_destroy, "ptx_comm_destroy") && sym(L.comm_n_ranks, "ptx_comm_n_ranks") &&
                  sym(L.allgather_digests, "ptx_allgather_digests") && sym(L.count_converged_digests, "ptx_count_converged_digests") &&
                  sym(L.result_download_logs, "ptx_result_download_logs") && sym(L.root_map, "ptx_root_map") && sym(L.root_maps_free, "ptx_root_maps_free") && sym(L.device_alloc, "ptx_device_alloc") && sym(L.device_free, "ptx_device_free") &&
                  sym(L.device_read, "ptx_device_read") && sym(L.resolve_cursors, "ptx_resolve_cursors") && sym(L.batch_append_device, "ptx_batch_append_device") &&
                  sym(L.sync_replicas, "ptx_sync_replicas") && sym(L.accumulate_patches, "ptx_accumulate_patches") && sym(L.check_patches, "ptx_check_patches") &&
                  sym(L.batch_at_versions, "ptx_batch_at_versions") && sym(L.strings_upload, "ptx_strings_upload") && sym(L.strings_free, "ptx_strings_free") &&
                  sym(L.result_text_range, "ptx_result_text_range") && sym(L.text_free, "ptx_text_free") && sym(L.result_find_text, "ptx_result_find_text") &&
                  sym(L.matches_free, "ptx_matches_free") && sym(L.result_text_slices, "ptx_result_text_slices") && sym(L.slices_free, "ptx_slices_free") &&
                  sym(L.text_view_create, "ptx_text_view_create") && sym(L.text_view_free, "ptx_text_view_free") && sym(L.view_find_text, "ptx_view_find_text") &&
                  sym(L.view_text_slices, "ptx_view_text_slices") && sym(L.view_find_snippets, "ptx_view_find_snippets") && sym(L.snippets_free, "ptx_snippets_free") &&
                  sym(L.view_replace_plan, "ptx_view_replace_plan") && sym(L.replace_plan_free, "ptx_replace_plan_free") &&
                  sym(L.view_mark_runs, "ptx_view_mark_runs") && sym(L.mark_runs_free, "ptx_mark_runs_free") && sym(L.view_mark_snippets, "ptx_view_mark_snippets") &&
                  sym(L.mark_snippets_free, "ptx_mark_snippets_free") && sym(L.view_find_in_marks, "ptx_view_find_in_marks");
        if (!ok) {
            dlclose(L.handle);
            L.handle = nullptr;
            return throw_msg(env, "libperitext_hip.so lacks a symbol include/peritext_hip.h declares");
        }
        if (L.abi_version() != PTX_ABI_VERSION) return throw_msg(env, "libperitext_hip.so ABI version mismatch");
    }
    napi_value v;
    NAPI_OK(napi_create_uint32(env, L.abi_version(), &v));
    return v;
}

napi_value Create(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    int32_t device = 0;
    uint32_t flags = 0;
    if (argc > 0) napi_get_value_int32(env, argv[0], &device);
    if (argc > 1) napi_get_value_uint32(env, argv[1], &flags);
    ptx_ctx* ctx = nullptr;
    const ptx_status st = L.create(device, flags, &ctx);
    if (st != PTX_OK) {
        char msg[1024];
        snprintf(msg, sizeof(msg), "ptx_create failed (status %d): %s", st, L.last_error(nullptr));
        return throw_msg(env, msg);
    }
    napi_value ext;
    NAPI_OK(napi_create_external(env, ctx, nullptr, nullptr, &ext));
    return ext;
}

ptx_ctx* ctx_of(napi_env env, napi_value v) {
    void* p = nullptr;
    if (napi_get_value_external(env, v, &p) != napi_ok) return nullptr;
    return (ptx_ctx*)p;
}

napi_value Destroy(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc ? ctx_of(env, argv[0]) : nullptr;
    if (ctx && L.handle) L.destroy(ctx);
    return nullptr;
}

/* typed-array property -> raw pointer + element count; expected element size is checked */
bool column(napi_env env, napi_value obj, const char* name, size_t elem, const void** ptr, size_t* count, bool optional = false) {
    napi_value v;
    bool has = false;
    if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) {
        *ptr = nullptr;
        *count = 0;
        return optional;
    }
    if (napi_get_named_property(env, obj, name, &v) != napi_ok) return false;
    bool is_ta = false;
    napi_is_typedarray(env, v, &is_ta);
    if (!is_ta) {
        *ptr = nullptr;
        *count = 0;
        return optional;
    }
    napi_typedarray_type type;
    size_t length = 0, offset = 0;
    void* data = nullptr;
    napi_value ab;
    if (napi_get_typedarray_info(env, v, &type, &length, &data, &ab, &offset) != napi_ok) return false;
    size_t es = 0;
    switch (type) {
        case napi_uint8_array: es = 1; break;
        case napi_uint16_array: es = 2; break;
        case napi_uint32_array: es = 4; break;
        case napi_biguint64_array: es = 8; break;
        default: return false;
    }
    if (es != elem) return false;
    *ptr = data;
    *count = length;
    return true;
}

napi_value make_u32(napi_env env, const void* src, size_t count) {
    napi_value ab, ta;
    void* data = nullptr;
    if (napi_create_arraybuffer(env, count * 4, &data, &ab) != napi_ok) return nullptr;
    if (count) memcpy(data, src, count * 4);
    if (napi_create_typedarray(env, napi_uint32_array, count, ab, 0, &ta) != napi_ok) return nullptr;
    return ta;
}

/* JS WireBatch (typed arrays, index.d.ts) -> ptx_batch pointing into their ArrayBuffers; false + pending exception on a malformed one */
bool read_batch(napi_env env, napi_value b, ptx_batch* out) {
    ptx_batch& pb = *out;
    memset(&pb, 0, sizeof(pb));
    size_t n_off = 0, n = 0, m = 0;
    const void* p = nullptr;
    if (!column(env, b, "logOff", 8, &p, &n_off)) return throw_msg(env, "batch.logOff must be a BigUint64Array"), false;
    pb.log_off = (const uint64_t*)p;
    if (n_off == 0) return throw_msg(env, "batch.logOff needs n_logs + 1 entries"), false;
    pb.n_logs = (uint32_t)(n_off - 1);
    pb.n_ops = pb.log_off[pb.n_logs];
    struct Col { const char* name; size_t elem; const void** dst; } cols[] = {
        {"opId", 8, (const void**)&pb.op_id},     {"refA", 8, (const void**)&pb.ref_a},         {"refB", 8, (const void**)&pb.ref_b},
        {"payload", 4, (const void**)&pb.payload}, {"action", 1, (const void**)&pb.action},     {"markType", 1, (const void**)&pb.mark_type},
        {"sideA", 1, (const void**)&pb.side_a},    {"sideB", 1, (const void**)&pb.side_b},
    };
    for (const Col& c : cols) {
        if (!column(env, b, c.name, c.elem, c.dst, &n) || n != pb.n_ops) {
            char msg[128];
            snprintf(msg, sizeof(msg), "batch.%s: typed array of %zu-byte elements with n_ops entries expected", c.name, c.elem);
            return throw_msg(env, msg), false;
        }
    }
    /* optional: per-log census (sizeof(ptx_log_hdr) / 4 = 10 u32 per log) — otherwise the library computes it on the device */
    if (column(env, b, "logHdr", 4, &p, &m, true) && p) {
        if (m != (size_t)pb.n_logs * (sizeof(ptx_log_hdr) / 4)) return throw_msg(env, "batch.logHdr: Uint32Array with 10 entries per log expected"), false;
        pb.log_hdr = (const ptx_log_hdr*)p;
    }
    /* optional: the Change envelope -> causal admission on the device (chgOff + chgHdr + chgEnv + maxActors, or none) */
    {
        size_t n_co = 0, n_h = 0, n_e = 0;
        const void *co = nullptr, *ch = nullptr, *ce = nullptr;
        uint32_t max_actors = 0;
        napi_value mv;
        bool has = false;
        if (napi_has_named_property(env, b, "maxActors", &has) == napi_ok && has && napi_get_named_property(env, b, "maxActors", &mv) == napi_ok)
            napi_get_value_uint32(env, mv, &max_actors);
        if (max_actors && column(env, b, "chgOff", 8, &co, &n_co, true) && co && column(env, b, "chgHdr", 4, &ch, &n_h, true) && ch &&
            column(env, b, "chgEnv", 2, &ce, &n_e, true) && ce) {
            const uint64_t nc = n_co == (size_t)pb.n_logs + 1 ? ((const uint64_t*)co)[pb.n_logs] : ~0ull;
            if (nc != n_h || nc * PTX_ENV_STRIDE(max_actors) != n_e) return throw_msg(env, "batch.chg*: inconsistent Change envelope columns"), false;
            pb.chg_off = (const uint64_t*)co;
            pb.chg_hdr = (const uint32_t*)ch;
            pb.chg_env = (const uint16_t*)ce;
            pb.max_actors = max_actors;
            /* optional wide column (ptx_batch.chg_env_hi): the high halves of chgEnv's values, same shape */
            size_t n_hi = 0;
            const void* hi = nullptr;
            if (column(env, b, "chgEnvHi", 2, &hi, &n_hi, true) && hi) {
                if (n_hi != n_e) return throw_msg(env, "batch.chgEnvHi: Uint16Array of the shape of chgEnv expected"), false;
                pb.chg_env_hi = (const uint16_t*)hi;
            }
        }
    }
    return true;
}


napi_value make_typed(napi_env env, napi_typedarray_type type, size_t elem, const void* src, size_t count) {
    napi_value ab, ta;
    void* data = nullptr;
    if (napi_create_arraybuffer(env, count * elem, &data, &ab) != napi_ok) return nullptr;
    if (count && src) memcpy(data, src, count * elem);
    if (napi_create_typedarray(env, type, count, ab, 0, &ta) != napi_ok) return nullptr;
    return ta;
}

/* ptx_batch in host memory -> JS WireBatch columns (copies) */
napi_value batch_to_js(napi_env env, const ptx_batch& b) {
    napi_value batch, v;
    if (napi_create_object(env, &batch) != napi_ok) return nullptr;
    const size_t Lg = b.n_logs, T = (size_t)b.n_ops, NC = b.chg_off ? (size_t)b.chg_off[Lg] : 0;
    struct { const char* name; napi_typedarray_type type; size_t elem; const void* src; size_t count; } cols[] = {
        {"logOff", napi_biguint64_array, 8, b.log_off, Lg + 1}, {"opId", napi_biguint64_array, 8, b.op_id, T}, {"refA", napi_biguint64_array, 8, b.ref_a, T},
        {"refB", napi_biguint64_array, 8, b.ref_b, T}, {"payload", napi_uint32_array, 4, b.payload, T}, {"action", napi_uint8_array, 1, b.action, T},
        {"markType", napi_uint8_array, 1, b.mark_type, T}, {"sideA", napi_uint8_array, 1, b.side_a, T}, {"sideB", napi_uint8_array, 1, b.side_b, T},
        {"logHdr", napi_uint32_array, 4, b.log_hdr, Lg * (sizeof(ptx_log_hdr) / 4)}, {"chgOff", napi_biguint64_array, 8, b.chg_off, Lg + 1},
        {"chgHdr", napi_uint32_array, 4, b.chg_hdr, NC}, {"chgEnv", napi_uint16_array, 2, b.chg_env, NC * PTX_ENV_STRIDE(b.max_actors)},
        {"chgEnvHi", napi_uint16_array, 2, b.chg_env_hi, b.chg_env_hi ? NC * PTX_ENV_STRIDE(b.max_actors) : 0},
    };
    for (auto& col : cols) {
        if (!col.src && col.count) continue;
        v = make_typed(env, col.type, col.elem, col.src, col.count);
        if (v) napi_set_named_property(env, batch, col.name, v);
    }
    napi_create_uint32(env, b.max_actors, &v);
    napi_set_named_property(env, batch, "maxActors", v);
    napi_create_uint32(env, b.n_logs, &v);
    napi_set_named_property(env, batch, "nLogs", v);
    napi_create_double(env, (double)b.n_ops, &v);
    napi_set_named_property(env, batch, "nOps", v);
    return batch;
}

/* the rows of a ptx_result (compact since ABI 7: log l's values at [valueOff[l], valueOff[l + 1]) ...) as typed arrays on `obj` */
static void result_rows_to_js(napi_env env, const ptx_result& res, napi_value obj) {
    napi_value v;
    static_assert(sizeof(ptx_log_result) == 48, "ptx_log_result layout");
    const size_t nl = (size_t)res.n_logs, n_off = nl + 1;
    v = make_u32(env, res.logs, nl * 12);
    if (v) napi_set_named_property(env, obj, "logs", v);
    v = make_u32(env, res.values, (size_t)res.value_off[nl]);
    if (v) napi_set_named_property(env, obj, "values", v);
    v = make_u32(env, res.spans, (size_t)res.span_off[nl] * 2);
    if (v) napi_set_named_property(env, obj, "spans", v);
    v = make_u32(env, res.cintervals, (size_t)res.cint_off[nl] * 3);
    if (v) napi_set_named_property(env, obj, "cintervals", v);
    const char* names[3] = {"valueOff", "spanOff", "cintOff"};
    const uint64_t* offs[3] = {res.value_off, res.span_off, res.cint_off};
    for (int k = 0; k < 3; ++k) {
        napi_value ab, ta;
        void* data = nullptr;
        if (napi_create_arraybuffer(env, n_off * 8, &data, &ab) == napi_ok && napi_create_typedarray(env, napi_biguint64_array, n_off, ab, 0, &ta) == napi_ok) {
            memcpy(data, offs[k], n_off * 8);
            napi_set_named_property(env, obj, names[k], ta);
        }
    }
    if (res.elem_rank) {
        v = make_u32(env, res.elem_rank, (size_t)res.n_rows);
        if (v) napi_set_named_property(env, obj, "elemRank", v);
    }
}

/* ptx_result (+ the patch streams) -> the JS result object; both are freed here */
napi_value result_to_js(napi_env env, ptx_result& res, ptx_patches* patp) {
    napi_value out;
    NAPI_OK(napi_create_object(env, &out));
    napi_value v;
    result_rows_to_js(env, res, out);
    L.result_free(&res);
    if (patp) {
        ptx_patches& pat = *patp;
        static_assert(sizeof(ptx_patch) == 16 && sizeof(ptx_patch_log) == 8, "ptx_patch layout");
        napi_value ab, ta;
        void* data = nullptr;
        const size_t n_off = (size_t)pat.n_logs + 1;
        if (napi_create_arraybuffer(env, n_off * 8, &data, &ab) == napi_ok && napi_create_typedarray(env, napi_biguint64_array, n_off, ab, 0, &ta) == napi_ok) {
            memcpy(data, pat.patch_off, n_off * 8);
            napi_set_named_property(env, out, "patchOff", ta);
        }
        v = make_u32(env, pat.logs, (size_t)pat.n_logs * 2);
        if (v) napi_set_named_property(env, out, "patchLogs", v);
        v = make_u32(env, pat.patches, (size_t)pat.patch_off[pat.n_logs] * 4);
        if (v) napi_set_named_property(env, out, "patches", v);
        L.patches_free(&pat);
    }
    return out;
}

napi_value ApplyMaterialize(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    if (argc < 2) return throw_msg(env, "applyMaterialize(ctx, batch[, wantPatches])");
    bool want_patches = false;
    if (argc > 2) napi_get_value_bool(env, argv[2], &want_patches);
    ptx_ctx* ctx = ctx_of(env, argv[0]);
    if (!ctx) return throw_msg(env, "applyMaterialize: bad context");
    ptx_batch pb;
    if (!read_batch(env, argv[1], &pb)) return nullptr;
    ptx_result res;
    ptx_patches pat;
    memset(&pat, 0, sizeof(pat));
    ptx_status st;
    if (!want_patches) {
        st = L.apply_materialize(ctx, &pb, &res);
    } else {
        /* the same in stages, the results stay in HBM for the replay that produces what every applyChange returns */
        ptx_dbatch* db = nullptr;
        ptx_dresult* dr = nullptr;
        st = L.batch_upload(ctx, &pb, &db);
        if (st == PTX_OK) st = L.result_alloc(ctx, db, &dr);
        if (st == PTX_OK) st = L.merge(ctx, db, dr);
        if (st == PTX_OK) st = L.sync(ctx);
        if (st == PTX_OK) st = L.result_download(ctx, db, dr, &res);
        if (st == PTX_OK) {
            st = L.replay_patches(ctx, db, dr, &pat);
            if (st != PTX_OK) L.result_free(&res);
        }
        if (dr) L.dresult_free(ctx, dr);
        if (db) L.batch_free(ctx, db);
    }
    if (st != PTX_OK) {
        char msg[1024];
        snprintf(msg, sizeof(msg), "ptx_apply_materialize failed (status %d): %s", st, L.last_error(ctx));
        return throw_msg(env, msg);
    }
    return result_to_js(env, res, want_patches ? &pat : nullptr);
}


/* ---- resident replicas (INTEGRATION.md "Resident replicas"): residentUpload(ctx, batch) -> handle; residentAppend(ctx, handle, more) -> new handle (the
 *      old one is released); residentApply(ctx, handle, wantPatches[, firstRow: Uint32Array]) -> the result object of applyMaterialize, the patch streams
 *      from firstRow[l] on; residentFree(ctx, handle) ---- */
ptx_dbatch* dbatch_of(napi_env env, napi_value v) {
    void* p = nullptr;
    if (napi_get_value_external(env, v, &p) != napi_ok) return nullptr;
    return (ptx_dbatch*)p;
}
napi_value lib_error(napi_env env, ptx_ctx* ctx, const char* what, ptx_status st) {
    char msg[1024];
    snprintf(msg, sizeof(msg), "%s failed (status %d): %s", what, st, L.last_error(ctx));
    return throw_msg(env, msg);
}
napi_value ResidentUpload(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 1 ? ctx_of(env, argv[0]) : nullptr;
    if (!ctx) return throw_msg(env, "residentUpload(ctx, batch)");
    ptx_batch pb;
    if (!read_batch(env, argv[1], &pb)) return nullptr;
    ptx_dbatch* db = nullptr;
    const ptx_status st = L.batch_upload(ctx, &pb, &db);
    if (st != PTX_OK) return lib_error(env, ctx, "ptx_batch_upload", st);
    napi_value ext;
    NAPI_OK(napi_create_external(env, db, nullptr, nullptr, &ext));
    return ext;
}
napi_value ResidentAppend(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 2 ? ctx_of(env, argv[0]) : nullptr;
    ptx_dbatch* base = ctx ? dbatch_of(env, argv[1]) : nullptr;
    if (!base) return throw_msg(env, "residentAppend(ctx, handle, moreBatch)");
    ptx_batch pb;
    if (!read_batch(env, argv[2], &pb)) return nullptr;
    ptx_dbatch* db = nullptr;
    const ptx_status st = L.batch_append(ctx, base, &pb, &db);
    if (st != PTX_OK) return lib_error(env, ctx, "ptx_batch_append", st);
    L.batch_free(ctx, base);
    napi_value ext;
    NAPI_OK(napi_create_external(env, db, nullptr, nullptr, &ext));
    return ext;
}
napi_value ResidentApply(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 4;
    napi_value argv[4];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 1 ? ctx_of(env, argv[0]) : nullptr;
    ptx_dbatch* db = ctx ? dbatch_of(env, argv[1]) : nullptr;
    if (!db) return throw_msg(env, "residentApply(ctx, handle[, wantPatches[, firstRow]])");
    bool want_patches = false;
    if (argc > 2) napi_get_value_bool(env, argv[2], &want_patches);
    const uint32_t* first = nullptr;
    if (argc > 3) {
        bool is_ta = false;
        napi_is_typedarray(env, argv[3], &is_ta);
        if (is_ta) {
            napi_typedarray_type type;
            size_t length = 0, offset = 0;
            void* data = nullptr;
            napi_value ab;
            if (napi_get_typedarray_info(env, argv[3], &type, &length, &data, &ab, &offset) != napi_ok || type != napi_uint32_array || length != L.batch_n_logs(db))
                return throw_msg(env, "residentApply: firstRow must be a Uint32Array with one entry per replica log");
            first = (const uint32_t*)data;
        }
    }
    ptx_dresult* dr = nullptr;
    ptx_result res;
    ptx_patches pat;
    memset(&pat, 0, sizeof(pat));
    ptx_status st = L.result_alloc(ctx, db, &dr);
    if (st == PTX_OK) st = L.merge(ctx, db, dr);
    if (st == PTX_OK) st = L.sync(ctx);
    if (st == PTX_OK) st = L.result_download(ctx, db, dr, &res);
    if (st == PTX_OK && want_patches) {
        st = L.replay_patches_from(ctx, db, dr, first, &pat);
        if (st != PTX_OK) L.result_free(&res);
    }
    if (dr) L.dresult_free(ctx, dr);
    if (st != PTX_OK) return lib_error(env, ctx, "residentApply (ptx_merge / ptx_replay_patches_from)", st);
    return result_to_js(env, res, want_patches ? &pat : nullptr);
}
napi_value ResidentFree(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 1 ? ctx_of(env, argv[0]) : nullptr;
    ptx_dbatch* db = ctx ? dbatch_of(env, argv[1]) : nullptr;
    if (db && L.handle) L.batch_free(ctx, db);
    return nullptr;
}

/* ---- document text assembled on the device (INTEGRATION.md "Text on the device"): stringsUpload(ctx, units: Uint16Array, off: BigUint64Array) -> handle of a
 *      resident string table (ptx_strings_upload); stringsFree(ctx, handle); resultText(ctx, batch, strings) -> the result object of applyMaterialize plus the
 *      text of every log (ptx_result_text_range): text: Uint16Array, textOff: BigUint64Array [nLogs + 1], textStatus: Uint32Array [nLogs], spanUnit: Uint32Array
 *      (beside spanOff), textKernelMs ---- */
ptx_dstrings* strings_of(napi_env env, napi_value v) {
    void* p = nullptr;
    if (napi_get_value_external(env, v, &p) != napi_ok) return nullptr;
    return (ptx_dstrings*)p;
}
/* the arrays of a ptx_text as properties of `obj`; the text is freed here */
static void text_to_js(napi_env env, ptx_text& t, napi_value obj) {
    const size_t nl = (size_t)t.n_logs;
    napi_value v = make_u32(env, t.status, nl);
    if (v) napi_set_named_property(env, obj, "textStatus", v);
    v = make_typed(env, napi_biguint64_array, 8, t.text_off, nl + 1);
    if (v) napi_set_named_property(env, obj, "textOff", v);
    v = make_typed(env, napi_uint16_array, 2, t.text, (size_t)t.text_off[nl]);
    if (v) napi_set_named_property(env, obj, "text", v);
    v = make_u32(env, t.span_unit, (size_t)t.span_off[nl]);
    if (v) napi_set_named_property(env, obj, "spanUnit", v);
    if (napi_create_double(env, (double)t.kernel_ms, &v) == napi_ok) napi_set_named_property(env, obj, "textKernelMs", v);
    L.text_free(&t);
}
napi_value StringsUpload(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 2 ? ctx_of(env, argv[0]) : nullptr;
    if (!ctx) return throw_msg(env, "stringsUpload(ctx, units: Uint16Array, off: BigUint64Array)");
    napi_typedarray_type tu, to;
    size_t nu = 0, no = 0, offset = 0;
    void *units = nullptr, *off = nullptr;
    napi_value ab;
    bool is_u = false, is_o = false;
    napi_is_typedarray(env, argv[1], &is_u);
    napi_is_typedarray(env, argv[2], &is_o);
    if (!is_u || !is_o || napi_get_typedarray_info(env, argv[1], &tu, &nu, &units, &ab, &offset) != napi_ok || napi_get_typedarray_info(env, argv[2], &to, &no, &off, &ab, &offset) != napi_ok ||
        tu != napi_uint16_array || to != napi_biguint64_array || no < 1 || no - 1 > 0xFFFFFFFFull || ((const uint64_t*)off)[no - 1] != nu)
        return throw_msg(env, "stringsUpload: units must be a Uint16Array and off a BigUint64Array of n + 1 offsets that end at its length");
    ptx_dstrings* ds = nullptr;
    const ptx_status st = L.strings_upload(ctx, (const uint16_t*)units, (const uint64_t*)off, (uint32_t)(no - 1), &ds);
    if (st != PTX_OK) return lib_error(env, ctx, "ptx_strings_upload", st);
    napi_value ext;
    NAPI_OK(napi_create_external(env, ds, nullptr, nullptr, &ext));
    return ext;
}
napi_value StringsFree(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 1 ? ctx_of(env, argv[0]) : nullptr;
    ptx_dstrings* ds = ctx ? strings_of(env, argv[1]) : nullptr;
    if (ds && L.handle) L.strings_free(ctx, ds);
    return nullptr;
}
napi_value ResultText(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 2 ? ctx_of(env, argv[0]) : nullptr;
    ptx_dstrings* ds = ctx ? strings_of(env, argv[2]) : nullptr;
    if (!ds) return throw_msg(env, "resultText(ctx, batch, strings)");
    ptx_batch pb;
    if (!read_batch(env, argv[1], &pb)) return nullptr;
    ptx_dbatch* db = nullptr;
    ptx_dresult* dr = nullptr;
    ptx_result res;
    ptx_text text;
    bool have_res = false;
    ptx_status st = L.batch_upload(ctx, &pb, &db);
    if (st == PTX_OK) st = L.result_alloc(ctx, db, &dr);
    if (st == PTX_OK) st = L.merge(ctx, db, dr);
    if (st == PTX_OK) st = L.result_download(ctx, db, dr, &res);
    have_res = st == PTX_OK;
    if (st == PTX_OK) st = L.result_text_range(ctx, db, dr, ds, 0, pb.n_logs, &text);
    std::string err = st != PTX_OK ? L.last_error(ctx) : "";
    if (dr) L.dresult_free(ctx, dr);
    if (db) L.batch_free(ctx, db);
    if (st != PTX_OK) {
        if (have_res) L.result_free(&res);
        char msg[1024];
        snprintf(msg, sizeof(msg), "resultText (ptx_merge / ptx_result_text_range) failed (status %d): %s", st, err.c_str());
        return throw_msg(env, msg);
    }
    napi_value out = result_to_js(env, res, nullptr);
    if (out) text_to_js(env, text, out);
    else L.text_free(&text);
    return out;
}

/* ---- find in the documents' text without downloading it (INTEGRATION.md "Find without downloading the text"): findText(ctx, batch, strings, pattern:
 *      Uint16Array, flags, maxHitsPerLog) uploads, merges and searches in one call (ptx_result_find_text) -> {status: Uint32Array [nLogs], nMatches: Uint32Array
 *      [nLogs], hitOff: BigUint64Array [nLogs + 1], hitUnit / hitStart / hitEnd: Uint32Array [hitOff[nLogs]], kernelMs} ---- */
napi_value FindText(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 6;
    napi_value argv[6];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 5 ? ctx_of(env, argv[0]) : nullptr;
    ptx_dstrings* ds = ctx ? strings_of(env, argv[2]) : nullptr;
    if (!ds) return throw_msg(env, "findText(ctx, batch, strings, pattern: Uint16Array, flags, maxHitsPerLog)");
    napi_typedarray_type tp;
    size_t np = 0, offset = 0;
    void* pat = nullptr;
    napi_value ab;
    bool is_p = false;
    napi_is_typedarray(env, argv[3], &is_p);
    uint32_t flags = 0, cap = 0;
    if (!is_p || napi_get_typedarray_info(env, argv[3], &tp, &np, &pat, &ab, &offset) != napi_ok || tp != napi_uint16_array || np > 0xFFFFFFFFull ||
        napi_get_value_uint32(env, argv[4], &flags) != napi_ok || napi_get_value_uint32(env, argv[5], &cap) != napi_ok)
        return throw_msg(env, "findText: pattern must be a Uint16Array, flags and maxHitsPerLog unsigned 32-bit numbers");
    ptx_batch pb;
    if (!read_batch(env, argv[1], &pb)) return nullptr;
    const uint16_t none = 0; /* (a zero-length typed array may come without storage: the library answers n_pattern == 0 itself) */
    ptx_dbatch* db = nullptr;
    ptx_dresult* dr = nullptr;
    ptx_matches m;
    ptx_status st = L.batch_upload(ctx, &pb, &db);
    if (st == PTX_OK) st = L.result_alloc(ctx, db, &dr);
    if (st == PTX_OK) st = L.merge(ctx, db, dr);
    if (st == PTX_OK) st = L.result_find_text(ctx, db, dr, ds, 0, pb.n_logs, np ? (const uint16_t*)pat : &none, (uint32_t)np, flags, cap, &m);
    std::string err = st != PTX_OK ? L.last_error(ctx) : "";
    if (dr) L.dresult_free(ctx, dr);
    if (db) L.batch_free(ctx, db);
    if (st != PTX_OK) {
        char msg[1024];
        snprintf(msg, sizeof(msg), "findText (ptx_merge / ptx_result_find_text) failed (status %d): %s", st, err.c_str());
        return throw_msg(env, msg);
    }
    const size_t nl = (size_t)m.n_logs, nh = (size_t)m.hit_off[nl];
    napi_value out = nullptr, v;
    if (napi_create_object(env, &out) == napi_ok) {
        if ((v = make_u32(env, m.status, nl))) napi_set_named_property(env, out, "status", v);
        if ((v = make_u32(env, m.n_matches, nl))) napi_set_named_property(env, out, "nMatches", v);
        if ((v = make_typed(env, napi_biguint64_array, 8, m.hit_off, nl + 1))) napi_set_named_property(env, out, "hitOff", v);
        if ((v = make_u32(env, m.hit_unit, nh))) napi_set_named_property(env, out, "hitUnit", v);
        if ((v = make_u32(env, m.hit_start, nh))) napi_set_named_property(env, out, "hitStart", v);
        if ((v = make_u32(env, m.hit_end, nh))) napi_set_named_property(env, out, "hitEnd", v);
        if (napi_create_double(env, (double)m.kernel_ms, &v) == napi_ok) napi_set_named_property(env, out, "kernelMs", v);
    }
    L.matches_free(&m);
    return out;
}

/* ---- the text and span rows of element ranges (INTEGRATION.md "Snippets without downloading the text"): textSlices(ctx, batch, strings, sliceOff: BigUint64Array
 *      [nLogs + 1], sliceStart, sliceEnd: Uint32Array) uploads, merges and cuts in one call (ptx_result_text_slices) -> the merge's compact rows (as
 *      applyMaterialize: the comment intervals resolve a row's comment ids) + {sliceStatus: Uint32Array [nLogs], elemStart / elemEnd: Uint32Array [nSlices],
 *      unitOff / sspanOff: BigUint64Array [nSlices + 1], sliceText: Uint16Array, sspans: Uint32Array (start, attr pairs), sspanUnit: Uint32Array, kernelMs} ---- */
static bool typed_arg(napi_env env, napi_value v, napi_typedarray_type want, void** data, size_t* n) {
    bool is = false;
    napi_typedarray_type tp;
    napi_value ab;
    size_t offset = 0;
    return napi_is_typedarray(env, v, &is) == napi_ok && is && napi_get_typedarray_info(env, v, &tp, n, data, &ab, &offset) == napi_ok && tp == want;
}
napi_value TextSlices(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 6;
    napi_value argv[6];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 5 ? ctx_of(env, argv[0]) : nullptr;
    ptx_dstrings* ds = ctx ? strings_of(env, argv[2]) : nullptr;
    if (!ds) return throw_msg(env, "textSlices(ctx, batch, strings, sliceOff: BigUint64Array, sliceStart: Uint32Array, sliceEnd: Uint32Array)");
    void *off = nullptr, *start = nullptr, *end = nullptr;
    size_t n_off = 0, n_start = 0, n_end = 0;
    if (!typed_arg(env, argv[3], napi_biguint64_array, &off, &n_off) || !typed_arg(env, argv[4], napi_uint32_array, &start, &n_start) || !typed_arg(env, argv[5], napi_uint32_array, &end, &n_end))
        return throw_msg(env, "textSlices: sliceOff must be a BigUint64Array, sliceStart and sliceEnd Uint32Arrays");
    ptx_batch pb;
    if (!read_batch(env, argv[1], &pb)) return nullptr;
    if (n_off != (size_t)pb.n_logs + 1 || n_start != n_end || ((const uint64_t*)off)[pb.n_logs] != n_start)
        return throw_msg(env, "textSlices: sliceOff holds nLogs + 1 offsets, the last one the length of sliceStart and sliceEnd");
    ptx_dbatch* db = nullptr;
    ptx_dresult* dr = nullptr;
    ptx_result res;
    ptx_slices m;
    bool have_res = false;
    ptx_status st = L.batch_upload(ctx, &pb, &db);
    if (st == PTX_OK) st = L.result_alloc(ctx, db, &dr);
    if (st == PTX_OK) st = L.merge(ctx, db, dr);
    if (st == PTX_OK) st = L.result_download(ctx, db, dr, &res);
    have_res = st == PTX_OK;
    if (st == PTX_OK) st = L.result_text_slices(ctx, db, dr, ds, 0, pb.n_logs, (const uint64_t*)off, n_start ? (const uint32_t*)start : nullptr, n_start ? (const uint32_t*)end : nullptr, &m);
    std::string err = st != PTX_OK ? L.last_error(ctx) : "";
    if (dr) L.dresult_free(ctx, dr);
    if (db) L.batch_free(ctx, db);
    if (st != PTX_OK) {
        if (have_res) L.result_free(&res);
        char msg[1024];
        snprintf(msg, sizeof(msg), "textSlices (ptx_merge / ptx_result_text_slices) failed (status %d): %s", st, err.c_str());
        return throw_msg(env, msg);
    }
    napi_value out = result_to_js(env, res, nullptr), v;
    if (out) {
        const size_t nl = (size_t)m.n_logs, ns = (size_t)m.n_slices, nu = (size_t)m.unit_off[ns], nr = (size_t)m.sspan_off[ns];
        if ((v = make_u32(env, m.status, nl))) napi_set_named_property(env, out, "sliceStatus", v);
        if ((v = make_u32(env, m.elem_start, ns))) napi_set_named_property(env, out, "elemStart", v);
        if ((v = make_u32(env, m.elem_end, ns))) napi_set_named_property(env, out, "elemEnd", v);
        if ((v = make_typed(env, napi_biguint64_array, 8, m.unit_off, ns + 1))) napi_set_named_property(env, out, "unitOff", v);
        if ((v = make_typed(env, napi_biguint64_array, 8, m.sspan_off, ns + 1))) napi_set_named_property(env, out, "sspanOff", v);
        if ((v = make_typed(env, napi_uint16_array, 2, m.text, nu))) napi_set_named_property(env, out, "sliceText", v);
        if ((v = make_u32(env, m.sspans, 2 * nr))) napi_set_named_property(env, out, "sspans", v);
        if ((v = make_u32(env, m.sspan_unit, nr))) napi_set_named_property(env, out, "sspanUnit", v);
        if (napi_create_double(env, (double)m.kernel_ms, &v) == napi_ok) napi_set_named_property(env, out, "kernelMs", v);
    }
    L.slices_free(&m);
    return out;
}

/* ---- a resident text view (INTEGRATION.md "Many searches against one merge"): viewCreate(ctx, batch, strings) uploads and merges, makes a view of every log
 *      (ptx_text_view_create) and returns the merge's compact rows (as applyMaterialize: the comment intervals resolve a row's comment ids) + {handle}.  The batch
 *      is freed before it returns and the strings may be freed by the caller: the handle keeps the merge's result and the view.  viewFindText(ctx, handle,
 *      pattern, flags, maxHitsPerLog) -> findText's object; viewTextSlices(ctx, handle, sliceOff, sliceStart, sliceEnd) -> textSlices' slice arrays;
 *      viewFindSnippets(ctx, handle, pattern, flags, maxHitsPerLog, before, after) -> both, the slices being one per listed hit (their sliceOff IS hitOff), and
 *      matchUnit: Uint32Array; viewFree(ctx, handle) ---- */
struct ViewHandle {
    ptx_dresult* dr = nullptr;
    ptx_dview* view = nullptr;
    uint32_t n_logs = 0;
};
static ViewHandle* view_of(napi_env env, napi_value v) {
    void* p = nullptr;
    if (napi_get_value_external(env, v, &p) != napi_ok) return nullptr;
    ViewHandle* h = (ViewHandle*)p;
    return h && h->view ? h : nullptr;
}
static bool pattern_arg(napi_env env, napi_value v, const uint16_t** pat, uint32_t* n) {
    static const uint16_t none = 0; /* (a zero-length typed array may come without storage: the library answers n_pattern == 0 itself) */
    void* data = nullptr;
    size_t len = 0;
    if (!typed_arg(env, v, napi_uint16_array, &data, &len) || len > 0xFFFFFFFFull) return false;
    *pat = len ? (const uint16_t*)data : &none;
    *n = (uint32_t)len;
    return true;
}
static void hits_to_js(napi_env env, napi_value out, const uint32_t* status, const uint32_t* n_matches, const uint64_t* hit_off, const uint32_t* hit_unit, const uint32_t* hit_start,
                       const uint32_t* hit_end, size_t nl) {
    const size_t nh = (size_t)hit_off[nl];
    napi_value v;
    if ((v = make_u32(env, status, nl))) napi_set_named_property(env, out, "status", v);
    if ((v = make_u32(env, n_matches, nl))) napi_set_named_property(env, out, "nMatches", v);
    if ((v = make_typed(env, napi_biguint64_array, 8, hit_off, nl + 1))) napi_set_named_property(env, out, "hitOff", v);
    if ((v = make_u32(env, hit_unit, nh))) napi_set_named_property(env, out, "hitUnit", v);
    if ((v = make_u32(env, hit_start, nh))) napi_set_named_property(env, out, "hitStart", v);
    if ((v = make_u32(env, hit_end, nh))) napi_set_named_property(env, out, "hitEnd", v);
}
static void cut_to_js(napi_env env, napi_value out, const uint32_t* status, size_t nl, size_t ns, const uint32_t* elem_start, const uint32_t* elem_end, const uint64_t* unit_off,
                      const uint64_t* sspan_off, const uint16_t* text, const ptx_span* sspans, const uint32_t* sspan_unit) {
    const size_t nu = (size_t)unit_off[ns], nr = (size_t)sspan_off[ns];
    napi_value v;
    if ((v = make_u32(env, status, nl))) napi_set_named_property(env, out, "sliceStatus", v);
    if ((v = make_u32(env, elem_start, ns))) napi_set_named_property(env, out, "elemStart", v);
    if ((v = make_u32(env, elem_end, ns))) napi_set_named_property(env, out, "elemEnd", v);
    if ((v = make_typed(env, napi_biguint64_array, 8, unit_off, ns + 1))) napi_set_named_property(env, out, "unitOff", v);
    if ((v = make_typed(env, napi_biguint64_array, 8, sspan_off, ns + 1))) napi_set_named_property(env, out, "sspanOff", v);
    if ((v = make_typed(env, napi_uint16_array, 2, text, nu))) napi_set_named_property(env, out, "sliceText", v);
    if ((v = make_u32(env, sspans, 2 * nr))) napi_set_named_property(env, out, "sspans", v);
    if ((v = make_u32(env, sspan_unit, nr))) napi_set_named_property(env, out, "sspanUnit", v);
}
napi_value ViewCreate(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 2 ? ctx_of(env, argv[0]) : nullptr;
    ptx_dstrings* ds = ctx ? strings_of(env, argv[2]) : nullptr;
    if (!ds) return throw_msg(env, "viewCreate(ctx, batch, strings)");
    ptx_batch pb;
    if (!read_batch(env, argv[1], &pb)) return nullptr;
    ptx_dbatch* db = nullptr;
    ViewHandle* h = new ViewHandle();
    h->n_logs = pb.n_logs;
    ptx_result res;
    bool have_res = false;
    ptx_status st = L.batch_upload(ctx, &pb, &db);
    if (st == PTX_OK) st = L.result_alloc(ctx, db, &h->dr);
    if (st == PTX_OK) st = L.merge(ctx, db, h->dr);
    if (st == PTX_OK) st = L.result_download(ctx, db, h->dr, &res);
    have_res = st == PTX_OK;
    if (st == PTX_OK) st = L.text_view_create(ctx, db, h->dr, ds, 0, pb.n_logs, &h->view);
    std::string err = st != PTX_OK ? L.last_error(ctx) : "";
    if (db) L.batch_free(ctx, db); /* the view reads nothing of the batch */
    napi_value out = st == PTX_OK ? result_to_js(env, res, nullptr) : nullptr, ext;
    if (st != PTX_OK && have_res) L.result_free(&res);
    if (out && napi_create_external(env, h, nullptr, nullptr, &ext) == napi_ok && napi_set_named_property(env, out, "handle", ext) == napi_ok) return out;
    if (h->view) L.text_view_free(ctx, h->view);
    if (h->dr) L.dresult_free(ctx, h->dr);
    delete h;
    if (st != PTX_OK) {
        char msg[1024];
        snprintf(msg, sizeof(msg), "viewCreate (ptx_merge / ptx_text_view_create) failed (status %d): %s", st, err.c_str());
        return throw_msg(env, msg);
    }
    return out;
}
napi_value ViewFree(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 1 ? ctx_of(env, argv[0]) : nullptr;
    ViewHandle* h = ctx ? view_of(env, argv[1]) : nullptr;
    if (h && L.handle) { /* the record itself stays (a second viewFree, or a query after it, finds no view and does nothing) */
        L.text_view_free(ctx, h->view);
        L.dresult_free(ctx, h->dr);
        h->view = nullptr;
        h->dr = nullptr;
    }
    return nullptr;
}
napi_value ViewFindText(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 5;
    napi_value argv[5];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 4 ? ctx_of(env, argv[0]) : nullptr;
    ViewHandle* h = ctx ? view_of(env, argv[1]) : nullptr;
    if (!h) return throw_msg(env, "viewFindText(ctx, handle, pattern: Uint16Array, flags, maxHitsPerLog): no live view");
    const uint16_t* pat = nullptr;
    uint32_t np = 0, flags = 0, cap = 0;
    if (!pattern_arg(env, argv[2], &pat, &np) || napi_get_value_uint32(env, argv[3], &flags) != napi_ok || napi_get_value_uint32(env, argv[4], &cap) != napi_ok)
        return throw_msg(env, "viewFindText: pattern must be a Uint16Array, flags and maxHitsPerLog unsigned 32-bit numbers");
    ptx_matches m;
    const ptx_status st = L.view_find_text(ctx, h->view, pat, np, flags, cap, &m);
    if (st != PTX_OK) return lib_error(env, ctx, "ptx_view_find_text", st);
    napi_value out = nullptr, v;
    if (napi_create_object(env, &out) == napi_ok) {
        hits_to_js(env, out, m.status, m.n_matches, m.hit_off, m.hit_unit, m.hit_start, m.hit_end, (size_t)m.n_logs);
        if (napi_create_double(env, (double)m.kernel_ms, &v) == napi_ok) napi_set_named_property(env, out, "kernelMs", v);
    }
    L.matches_free(&m);
    return out;
}
napi_value ViewTextSlices(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 5;
    napi_value argv[5];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 4 ? ctx_of(env, argv[0]) : nullptr;
    ViewHandle* h = ctx ? view_of(env, argv[1]) : nullptr;
    if (!h) return throw_msg(env, "viewTextSlices(ctx, handle, sliceOff: BigUint64Array, sliceStart: Uint32Array, sliceEnd: Uint32Array): no live view");
    void *off = nullptr, *start = nullptr, *end = nullptr;
    size_t n_off = 0, n_start = 0, n_end = 0;
    if (!typed_arg(env, argv[2], napi_biguint64_array, &off, &n_off) || !typed_arg(env, argv[3], napi_uint32_array, &start, &n_start) || !typed_arg(env, argv[4], napi_uint32_array, &end, &n_end))
        return throw_msg(env, "viewTextSlices: sliceOff must be a BigUint64Array, sliceStart and sliceEnd Uint32Arrays");
    if (n_off != (size_t)h->n_logs + 1 || n_start != n_end || ((const uint64_t*)off)[h->n_logs] != n_start)
        return throw_msg(env, "viewTextSlices: sliceOff holds nLogs + 1 offsets, the last one the length of sliceStart and sliceEnd");
    ptx_slices m;
    const ptx_status st = L.view_text_slices(ctx, h->view, (const uint64_t*)off, n_start ? (const uint32_t*)start : nullptr, n_start ? (const uint32_t*)end : nullptr, &m);
    if (st != PTX_OK) return lib_error(env, ctx, "ptx_view_text_slices", st);
    napi_value out = nullptr, v;
    if (napi_create_object(env, &out) == napi_ok) {
        cut_to_js(env, out, m.status, (size_t)m.n_logs, (size_t)m.n_slices, m.elem_start, m.elem_end, m.unit_off, m.sspan_off, m.text, m.sspans, m.sspan_unit);
        if (napi_create_double(env, (double)m.kernel_ms, &v) == napi_ok) napi_set_named_property(env, out, "kernelMs", v);
    }
    L.slices_free(&m);
    return out;
}
napi_value ViewFindSnippets(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 7;
    napi_value argv[7];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 6 ? ctx_of(env, argv[0]) : nullptr;
    ViewHandle* h = ctx ? view_of(env, argv[1]) : nullptr;
    if (!h) return throw_msg(env, "viewFindSnippets(ctx, handle, pattern: Uint16Array, flags, maxHitsPerLog, before, after): no live view");
    const uint16_t* pat = nullptr;
    uint32_t np = 0, flags = 0, cap = 0, before = 0, after = 0;
    if (!pattern_arg(env, argv[2], &pat, &np) || napi_get_value_uint32(env, argv[3], &flags) != napi_ok || napi_get_value_uint32(env, argv[4], &cap) != napi_ok ||
        napi_get_value_uint32(env, argv[5], &before) != napi_ok || napi_get_value_uint32(env, argv[6], &after) != napi_ok)
        return throw_msg(env, "viewFindSnippets: pattern must be a Uint16Array, flags, maxHitsPerLog, before and after unsigned 32-bit numbers");
    ptx_snippets m;
    const ptx_status st = L.view_find_snippets(ctx, h->view, pat, np, flags, cap, before, after, &m);
    if (st != PTX_OK) return lib_error(env, ctx, "ptx_view_find_snippets", st);
    napi_value out = nullptr, v;
    if (napi_create_object(env, &out) == napi_ok) {
        hits_to_js(env, out, m.status, m.n_matches, m.hit_off, m.hit_unit, m.hit_start, m.hit_end, (size_t)m.n_logs);
        cut_to_js(env, out, m.status, (size_t)m.n_logs, (size_t)m.n_slices, m.elem_start, m.elem_end, m.unit_off, m.sspan_off, m.text, m.sspans, m.sspan_unit);
        if ((v = make_u32(env, m.match_unit, (size_t)m.n_slices))) napi_set_named_property(env, out, "matchUnit", v);
        if (napi_create_double(env, (double)m.kernel_ms, &v) == napi_ok) napi_set_named_property(env, out, "kernelMs", v);
    }
    L.snippets_free(&m);
    return out;
}
/* ---- the view queried by format: viewMarkRuns(ctx, handle, markType, id, maxRunsPerLog) -> {status, nRuns, runOff, runStart, runEnd, runId, runUnit, runLen};
 *      viewMarkSnippets(ctx, handle, markType, id, maxRunsPerLog, before, after) -> the same and the slice arrays of one slice per listed run (their sliceOff IS
 *      runOff) with matchUnit; viewFindInMarks(ctx, handle, pattern, flags, markType, id, maxHitsPerLog) -> viewFindText's object, of the contained hits ---- */
static void runs_to_js(napi_env env, napi_value out, const uint32_t* status, const uint32_t* n_runs, const uint64_t* run_off, const uint32_t* run_start, const uint32_t* run_end,
                       const uint32_t* run_id, const uint32_t* run_unit, const uint32_t* run_len, size_t nl) {
    const size_t nr = (size_t)run_off[nl];
    napi_value v;
    if ((v = make_u32(env, status, nl))) napi_set_named_property(env, out, "status", v);
    if ((v = make_u32(env, n_runs, nl))) napi_set_named_property(env, out, "nRuns", v);
    if ((v = make_typed(env, napi_biguint64_array, 8, run_off, nl + 1))) napi_set_named_property(env, out, "runOff", v);
    if ((v = make_u32(env, run_start, nr))) napi_set_named_property(env, out, "runStart", v);
    if ((v = make_u32(env, run_end, nr))) napi_set_named_property(env, out, "runEnd", v);
    if ((v = make_u32(env, run_id, nr))) napi_set_named_property(env, out, "runId", v);
    if ((v = make_u32(env, run_unit, nr))) napi_set_named_property(env, out, "runUnit", v);
    if ((v = make_u32(env, run_len, nr))) napi_set_named_property(env, out, "runLen", v);
}
static bool u32_args(napi_env env, const napi_value* argv, uint32_t* out, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (napi_get_value_uint32(env, argv[i], &out[i]) != napi_ok) return false;
    return true;
}
napi_value ViewMarkRuns(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 5;
    napi_value argv[5];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 4 ? ctx_of(env, argv[0]) : nullptr;
    ViewHandle* h = ctx ? view_of(env, argv[1]) : nullptr;
    if (!h) return throw_msg(env, "viewMarkRuns(ctx, handle, markType, id, maxRunsPerLog): no live view");
    uint32_t a[3];
    if (!u32_args(env, argv + 2, a, 3)) return throw_msg(env, "viewMarkRuns: markType, id and maxRunsPerLog must be unsigned 32-bit numbers");
    ptx_mark_runs m;
    const ptx_status st = L.view_mark_runs(ctx, h->view, a[0], a[1], a[2], &m);
    if (st != PTX_OK) return lib_error(env, ctx, "ptx_view_mark_runs", st);
    napi_value out = nullptr, v;
    if (napi_create_object(env, &out) == napi_ok) {
        runs_to_js(env, out, m.status, m.n_runs, m.run_off, m.run_start, m.run_end, m.run_id, m.run_unit, m.run_len, (size_t)m.n_logs);
        if (napi_create_double(env, (double)m.kernel_ms, &v) == napi_ok) napi_set_named_property(env, out, "kernelMs", v);
    }
    L.mark_runs_free(&m);
    return out;
}
napi_value ViewMarkSnippets(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 7;
    napi_value argv[7];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 6 ? ctx_of(env, argv[0]) : nullptr;
    ViewHandle* h = ctx ? view_of(env, argv[1]) : nullptr;
    if (!h) return throw_msg(env, "viewMarkSnippets(ctx, handle, markType, id, maxRunsPerLog, before, after): no live view");
    uint32_t a[5];
    if (!u32_args(env, argv + 2, a, 5)) return throw_msg(env, "viewMarkSnippets: markType, id, maxRunsPerLog, before and after must be unsigned 32-bit numbers");
    ptx_mark_snippets m;
    const ptx_status st = L.view_mark_snippets(ctx, h->view, a[0], a[1], a[2], a[3], a[4], &m);
    if (st != PTX_OK) return lib_error(env, ctx, "ptx_view_mark_snippets", st);
    napi_value out = nullptr, v;
    if (napi_create_object(env, &out) == napi_ok) {
        runs_to_js(env, out, m.status, m.n_runs, m.run_off, m.run_start, m.run_end, m.run_id, m.run_unit, m.run_len, (size_t)m.n_logs);
        cut_to_js(env, out, m.status, (size_t)m.n_logs, (size_t)m.n_slices, m.elem_start, m.elem_end, m.unit_off, m.sspan_off, m.text, m.sspans, m.sspan_unit);
        if ((v = make_u32(env, m.match_unit, (size_t)m.n_slices))) napi_set_named_property(env, out, "matchUnit", v);
        if (napi_create_double(env, (double)m.kernel_ms, &v) == napi_ok) napi_set_named_property(env, out, "kernelMs", v);
    }
    L.mark_snippets_free(&m);
    return out;
}
napi_value ViewFindInMarks(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 7;
    napi_value argv[7];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 6 ? ctx_of(env, argv[0]) : nullptr;
    ViewHandle* h = ctx ? view_of(env, argv[1]) : nullptr;
    if (!h) return throw_msg(env, "viewFindInMarks(ctx, handle, pattern: Uint16Array, flags, markType, id, maxHitsPerLog): no live view");
    const uint16_t* pat = nullptr;
    uint32_t np = 0, a[4];
    if (!pattern_arg(env, argv[2], &pat, &np) || !u32_args(env, argv + 3, a, 4))
        return throw_msg(env, "viewFindInMarks: pattern must be a Uint16Array, flags, markType, id and maxHitsPerLog unsigned 32-bit numbers");
    ptx_matches m;
    const ptx_status st = L.view_find_in_marks(ctx, h->view, pat, np, a[0], a[1], a[2], a[3], &m);
    if (st != PTX_OK) return lib_error(env, ctx, "ptx_view_find_in_marks", st);
    napi_value out = nullptr, v;
    if (napi_create_object(env, &out) == napi_ok) {
        hits_to_js(env, out, m.status, m.n_matches, m.hit_off, m.hit_unit, m.hit_start, m.hit_end, (size_t)m.n_logs);
        if (napi_create_double(env, (double)m.kernel_ms, &v) == napi_ok) napi_set_named_property(env, out, "kernelMs", v);
    }
    L.matches_free(&m);
    return out;
}
/* viewReplacePlan(ctx, handle, pattern, flags, nReplacement) -> the plan of ptx_view_replace_plan over every log of the view: status, nMatches, nChosen, nReplaced
 * (Uint32Array per log), chgOff, opOff (BigUint64Array), action (Uint8Array), index, count (Uint32Array).  The value ids of the inserts are not the addon's
 * business: index.js writes the replacement's strings into the InputOperations itself, as bridge.ts:445 does */
napi_value ViewReplacePlan(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 5;
    napi_value argv[5];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 4 ? ctx_of(env, argv[0]) : nullptr;
    ViewHandle* h = ctx ? view_of(env, argv[1]) : nullptr;
    if (!h) return throw_msg(env, "viewReplacePlan(ctx, handle, pattern: Uint16Array, flags, nReplacement): no live view");
    const uint16_t* pat = nullptr;
    uint32_t np = 0, flags = 0, nrep = 0;
    if (!pattern_arg(env, argv[2], &pat, &np) || napi_get_value_uint32(env, argv[3], &flags) != napi_ok || napi_get_value_uint32(env, argv[4], &nrep) != napi_ok)
        return throw_msg(env, "viewReplacePlan: pattern must be a Uint16Array, flags and nReplacement unsigned 32-bit numbers");
    std::vector<uint32_t> ids(nrep <= PTX_CHANGE_ROWS_MAX ? nrep : 1u, 0u); /* (a longer replacement is the library's PTX_ERR_INVALID_ARG) */
    ptx_replace_plan m;
    const ptx_status st = L.view_replace_plan(ctx, h->view, pat, np, flags, ids.data(), nrep, h->n_logs, &m);
    if (st != PTX_OK) return lib_error(env, ctx, "ptx_view_replace_plan", st);
    napi_value out = nullptr, v;
    if (napi_create_object(env, &out) == napi_ok) {
        const size_t nl = (size_t)m.n_logs, nb = (size_t)m.ops.n_logs, nc = (size_t)m.ops.chg_off[nb], ni = (size_t)m.ops.op_off[nc];
        if ((v = make_u32(env, m.status, nl))) napi_set_named_property(env, out, "status", v);
        if ((v = make_u32(env, m.n_matches, nl))) napi_set_named_property(env, out, "nMatches", v);
        if ((v = make_u32(env, m.n_chosen, nl))) napi_set_named_property(env, out, "nChosen", v);
        if ((v = make_u32(env, m.n_replaced, nl))) napi_set_named_property(env, out, "nReplaced", v);
        if ((v = make_typed(env, napi_biguint64_array, 8, m.ops.chg_off, nb + 1))) napi_set_named_property(env, out, "chgOff", v);
        if ((v = make_typed(env, napi_biguint64_array, 8, m.ops.op_off, nc + 1))) napi_set_named_property(env, out, "opOff", v);
        if ((v = make_typed(env, napi_uint8_array, 1, m.ops.action, ni))) napi_set_named_property(env, out, "action", v);
        if ((v = make_u32(env, m.ops.index, ni))) napi_set_named_property(env, out, "index", v);
        if ((v = make_u32(env, m.ops.count, ni))) napi_set_named_property(env, out, "count", v);
        if (napi_create_double(env, (double)m.kernel_ms, &v) == napi_ok) napi_set_named_property(env, out, "kernelMs", v);
    }
    L.replace_plan_free(&m);
    return out;
}

uint32_t u32_prop(napi_env env, napi_value obj, const char* name, uint32_t dflt) {
    napi_value v;
    bool has = false;
    uint32_t out = dflt;
    if (napi_has_named_property(env, obj, name, &has) == napi_ok && has && napi_get_named_property(env, obj, name, &v) == napi_ok) napi_get_value_uint32(env, v, &out);
    return out;
}

/* generate(ctx, cfg): ptx_generate (on-device change(), the fuzzer workload) + merge of what it made, all resident; returns the
 * op-log columns (ptx_batch_download), the comment-id counts per document and the merge result */
napi_value Generate(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 1 ? ctx_of(env, argv[0]) : nullptr;
    if (!ctx) return throw_msg(env, "generate(ctx, cfg)");
    napi_value c = argv[1];
    ptx_gen_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.replicas = u32_prop(env, c, "replicas", 1);
    cfg.ops_per_log = u32_prop(env, c, "opsPerLog", 0);
    cfg.seed = u32_prop(env, c, "seed", 1);
    cfg.first_doc = u32_prop(env, c, "firstDoc", 0);
    cfg.n_docs = u32_prop(env, c, "nDocs", 1);
    cfg.list_cap = u32_prop(env, c, "listCap", 0);
    napi_value arr;
    uint32_t len = 0;
    if (napi_get_named_property(env, c, "mix", &arr) != napi_ok || napi_get_array_length(env, arr, &len) != napi_ok || len != 4) return throw_msg(env, "cfg.mix: [insert, delete, addMark, removeMark] percent");
    for (uint32_t i = 0; i < 4; ++i) {
        napi_value e;
        napi_get_element(env, arr, i, &e);
        napi_get_value_uint32(env, e, &cfg.mix[i]);
    }
    if (napi_get_named_property(env, c, "markTypes", &arr) != napi_ok || napi_get_array_length(env, arr, &len) != napi_ok || len > 4) return throw_msg(env, "cfg.markTypes: up to four PTX_MARK_* codes");
    cfg.n_mark_types = len;
    for (uint32_t i = 0; i < len; ++i) {
        napi_value e;
        uint32_t t = 0;
        napi_get_element(env, arr, i, &e);
        napi_get_value_uint32(env, e, &t);
        cfg.mark_types[i] = (uint8_t)t;
    }
    {
        napi_value tv;
        bool has = false;
        size_t tl = 0;
        if (napi_has_named_property(env, c, "initialText", &has) == napi_ok && has && napi_get_named_property(env, c, "initialText", &tv) == napi_ok)
            napi_get_value_string_utf8(env, tv, cfg.initial_text, sizeof(cfg.initial_text), &tl);
    }
    ptx_dbatch* db = nullptr;
    ptx_dresult* dr = nullptr;
    ptx_gen_info gi;
    ptx_host_batch hb;
    ptx_result res;
    memset(&hb, 0, sizeof(hb));
    ptx_status st = L.generate(ctx, &cfg, &db, &gi);
    if (st != PTX_OK) {
        char msg[1024];
        snprintf(msg, sizeof(msg), "ptx_generate failed (status %d): %s", st, L.last_error(ctx));
        return throw_msg(env, msg);
    }
    st = L.batch_download(ctx, db, &hb);
    if (st == PTX_OK) st = L.result_alloc(ctx, db, &dr);
    if (st == PTX_OK) st = L.merge(ctx, db, dr);
    if (st == PTX_OK) st = L.sync(ctx);
    bool have_res = false;
    if (st == PTX_OK) {
        st = L.result_download(ctx, db, dr, &res);
        have_res = st == PTX_OK;
    }
    if (dr) L.dresult_free(ctx, dr);
    L.batch_free(ctx, db);
    if (st != PTX_OK) {
        char msg[1024];
        snprintf(msg, sizeof(msg), "generate: merge of the generated batch failed (status %d): %s", st, L.last_error(ctx));
        if (hb.owner) L.host_batch_free(&hb);
        L.gen_info_free(&gi);
        return throw_msg(env, msg);
    }
    napi_value out, batch, result, v;
    NAPI_OK(napi_create_object(env, &out));
    NAPI_OK(napi_create_object(env, &result));
    batch = batch_to_js(env, hb.b);
    if (!batch) return throw_msg(env, "generate: cannot build the batch object");
    napi_set_named_property(env, out, "batch", batch);
    v = make_u32(env, gi.n_comments, gi.n_docs);
    if (v) napi_set_named_property(env, out, "nComments", v);
    napi_create_double(env, (double)gi.kernel_ms, &v);
    napi_set_named_property(env, out, "kernelMs", v);
    if (have_res) {
        result_rows_to_js(env, res, result);
        L.result_free(&res);
        napi_set_named_property(env, out, "result", result);
    }
    L.host_batch_free(&hb);
    L.gen_info_free(&gi);
    return out;
}

/* change(ctx, batch, inputOps): Micromerge.change for many replicas (ptx_change).  `batch` = the replica logs applied so far
 * (WireBatch with the Change envelope), inputOps = {chgOff, opOff: BigUint64Array, action, markType: Uint8Array, index, count,
 * payload, values, actor: Uint32Array, maxActors}.  Upload, merge, ptx_change, download of what was made.
 * Returns {batch: WireBatch columns of the new Changes only, status: Uint32Array per log}. */
napi_value Change(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 2 ? ctx_of(env, argv[0]) : nullptr;
    if (!ctx) return throw_msg(env, "change(ctx, batch | resident handle, inputOps)");
    /* the replicas: a host batch (encoded, uploaded and merged here), or the handle of a RESIDENT batch (residentUpload / residentAppend): then nothing of the
     * document goes up — the InputOperations are resolved against the logs in HBM, the Changes made are appended to them on the device and the new handle
     * comes back beside the made rows (the old one is released) */
    napi_valuetype vt;
    const bool resident = napi_typeof(env, argv[1], &vt) == napi_ok && vt == napi_external;
    ptx_batch pb;
    memset(&pb, 0, sizeof(pb));
    ptx_dbatch* rdb = resident ? dbatch_of(env, argv[1]) : nullptr;
    if (resident) {
        if (!rdb) return throw_msg(env, "change: bad resident handle");
        pb.n_logs = L.batch_n_logs(rdb);
    } else if (!read_batch(env, argv[1], &pb)) return nullptr;
    napi_value io = argv[2];
    ptx_input_ops in;
    memset(&in, 0, sizeof(in));
    size_t n_co = 0, n_oo = 0, n = 0, n_ops = 0, n_act = 0;
    const void* p = nullptr;
    if (!column(env, io, "chgOff", 8, &p, &n_co) || n_co != (size_t)pb.n_logs + 1) return throw_msg(env, "inputOps.chgOff: BigUint64Array with n_logs + 1 entries expected");
    in.chg_off = (const uint64_t*)p;
    if (!column(env, io, "opOff", 8, &p, &n_oo) || n_oo != (size_t)in.chg_off[pb.n_logs] + 1) return throw_msg(env, "inputOps.opOff: BigUint64Array with n_changes + 1 entries expected");
    in.op_off = (const uint64_t*)p;
    n_ops = (size_t)in.op_off[n_oo - 1];
    struct Col { const char* name; size_t elem; const void** dst; } cols[] = {
        {"action", 1, (const void**)&in.action}, {"markType", 1, (const void**)&in.mark_type}, {"index", 4, (const void**)&in.index},
        {"count", 4, (const void**)&in.count},   {"payload", 4, (const void**)&in.payload},
    };
    for (const Col& c : cols)
        if (!column(env, io, c.name, c.elem, c.dst, &n) || n != n_ops) return throw_msg(env, "inputOps: a column does not have one entry per InputOperation");
    if (!column(env, io, "values", 4, &p, &n)) return throw_msg(env, "inputOps.values must be a Uint32Array");
    in.values = (const uint32_t*)p;
    in.n_values = n;
    if (!column(env, io, "actor", 4, &p, &n_act) || n_act != pb.n_logs) return throw_msg(env, "inputOps.actor: Uint32Array with one entry per log expected");
    in.actor = (const uint32_t*)p;
    in.n_logs = pb.n_logs;
    in.max_actors = u32_prop(env, io, "maxActors", pb.max_actors);
    if (resident && in.max_actors == 0) return throw_msg(env, "change on a resident handle: inputOps.maxActors is needed");
    ptx_dbatch *db = nullptr, *made = nullptr;
    ptx_dresult* dr = nullptr;
    ptx_host_batch hb;
    memset(&hb, 0, sizeof(hb));
    napi_value status_arr = nullptr;
    void* status_data = nullptr;
    {
        napi_value ab;
        if (napi_create_arraybuffer(env, (size_t)pb.n_logs * 4, &status_data, &ab) != napi_ok ||
            napi_create_typedarray(env, napi_uint32_array, pb.n_logs, ab, 0, &status_arr) != napi_ok)
            return throw_msg(env, "change: cannot allocate the status array");
    }
    ptx_dbatch* after = nullptr;
    ptx_status st = resident ? PTX_OK : L.batch_upload(ctx, &pb, &db);
    if (resident) db = rdb;
    if (st == PTX_OK) st = L.result_alloc(ctx, db, &dr);
    if (st == PTX_OK) st = L.merge(ctx, db, dr);
    if (st == PTX_OK) st = L.sync(ctx);
    if (st == PTX_OK) st = L.change(ctx, db, dr, &in, &made, (uint32_t*)status_data);
    if (st == PTX_OK) st = L.batch_download(ctx, made, &hb);
    if (st == PTX_OK && resident) st = L.batch_append_device(ctx, db, made, &after); /* the replicas after the edit: still resident, nothing re-uploaded */
    if (dr) L.dresult_free(ctx, dr);
    if (db && !resident) L.batch_free(ctx, db);
    if (made) L.batch_free(ctx, made);
    if (st != PTX_OK) {
        char msg[1024];
        snprintf(msg, sizeof(msg), "ptx_change failed (status %d): %s", st, L.last_error(ctx));
        if (hb.owner) L.host_batch_free(&hb);
        return throw_msg(env, msg);
    }
    napi_value out, batch = batch_to_js(env, hb.b);
    L.host_batch_free(&hb);
    if (!batch || napi_create_object(env, &out) != napi_ok) {
        if (after) L.batch_free(ctx, after); /* the session keeps its old handle (rdb): still valid */
        return throw_msg(env, "change: cannot build the result object");
    }
    napi_set_named_property(env, out, "batch", batch);
    napi_set_named_property(env, out, "status", status_arr);
    if (resident) {
        /* the new handle first, the old batch only once the result object holds it: a failure here must leave the session with a live handle */
        napi_value ext;
        if (napi_create_external(env, after, nullptr, nullptr, &ext) != napi_ok || napi_set_named_property(env, out, "handle", ext) != napi_ok) {
            L.batch_free(ctx, after);
            return throw_msg(env, "change: cannot hand out the resident batch");
        }
        L.batch_free(ctx, rdb); /* superseded by `after` */
    }
    return out;
}

/* syncReplicas(ctx, batch, {src, dst: Uint32Array, maxAttempts}): getMissingChanges + applyChanges (reference/test/merge.ts:4-38) for many replica pairs
 * (ptx_sync_replicas).  `batch` = the replica logs applied so far (WireBatch with the Change envelope); pair p = logs (src[p], dst[p]).  Upload, sync, download
 * of `more`.  Returns {batch: WireBatch columns of `more` (log dst[p] = what the target lacks, in the order it admits it), status: Uint32Array per pair}. */
napi_value SyncReplicas(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 2 ? ctx_of(env, argv[0]) : nullptr;
    if (!ctx) return throw_msg(env, "syncReplicas(ctx, batch, {src, dst, maxAttempts})");
    ptx_batch pb;
    if (!read_batch(env, argv[1], &pb)) return nullptr;
    const void *src = nullptr, *dst = nullptr;
    size_t n_src = 0, n_dst = 0;
    if (!column(env, argv[2], "src", 4, &src, &n_src) || !column(env, argv[2], "dst", 4, &dst, &n_dst) || n_src != n_dst || n_src > 0xFFFFFFFFull)
        return throw_msg(env, "syncReplicas: src and dst must be Uint32Arrays of one length");
    const uint32_t max_attempts = u32_prop(env, argv[2], "maxAttempts", 10001u);
    napi_value status_arr = nullptr, ab;
    void* status_data = nullptr;
    if (napi_create_arraybuffer(env, n_src * 4, &status_data, &ab) != napi_ok || napi_create_typedarray(env, napi_uint32_array, n_src, ab, 0, &status_arr) != napi_ok)
        return throw_msg(env, "syncReplicas: cannot allocate the status array");
    ptx_dbatch *db = nullptr, *more = nullptr;
    ptx_host_batch hb;
    memset(&hb, 0, sizeof(hb));
    uint32_t none = 0; /* (a zero-length ArrayBuffer may come without storage) */
    ptx_status st = L.batch_upload(ctx, &pb, &db);
    if (st == PTX_OK) st = L.sync_replicas(ctx, db, (uint32_t)n_src, n_src ? (const uint32_t*)src : &none, n_src ? (const uint32_t*)dst : &none, max_attempts, &more, n_src ? (uint32_t*)status_data : &none);
    if (st == PTX_OK) st = L.batch_download(ctx, more, &hb);
    if (more) L.batch_free(ctx, more);
    if (db) L.batch_free(ctx, db);
    if (st != PTX_OK) {
        char msg[1024];
        snprintf(msg, sizeof(msg), "ptx_sync_replicas failed (status %d): %s", st, L.last_error(ctx));
        if (hb.owner) L.host_batch_free(&hb);
        return throw_msg(env, msg);
    }
    napi_value out, batch = batch_to_js(env, hb.b);
    L.host_batch_free(&hb);
    if (!batch || napi_create_object(env, &out) != napi_ok) return throw_msg(env, "syncReplicas: cannot build the result object");
    napi_set_named_property(env, out, "batch", batch);
    napi_set_named_property(env, out, "status", status_arr);
    return out;
}

/* batchAtVersions(ctx, batch, {src: Uint32Array, clocks | prefix: Uint32Array, thenRest, diff}): the replica logs of `batch` at past versions
 * (ptx_batch_at_versions).  Cut c reads log src[c]; clocks holds maxActors entries per cut (0xFFFFFFFF = every change of the actor), prefix one.  Upload, cut,
 * merge of the cut logs and — diff — ptx_replay_patches_from at the kept rows (thenRest is implied: the stream from the version to the present).  Returns
 * {batch: WireBatch columns of the cut logs, status, nKept, firstRow, clocksOut: Uint32Arrays, result: the result object of applyMaterialize for the cut logs}. */
napi_value BatchAtVersions(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 2 ? ctx_of(env, argv[0]) : nullptr;
    if (!ctx) return throw_msg(env, "batchAtVersions(ctx, batch, {src, clocks | prefix, thenRest, diff})");
    ptx_batch pb;
    if (!read_batch(env, argv[1], &pb)) return nullptr;
    const void *src = nullptr, *clocks = nullptr, *prefix = nullptr;
    size_t n = 0, n_clocks = 0, n_prefix = 0;
    if (!column(env, argv[2], "src", 4, &src, &n) || n > 0xFFFFFFFFull) return throw_msg(env, "batchAtVersions: src must be a Uint32Array");
    if (!column(env, argv[2], "clocks", 4, &clocks, &n_clocks, true) || !column(env, argv[2], "prefix", 4, &prefix, &n_prefix, true))
        return throw_msg(env, "batchAtVersions: clocks / prefix must be Uint32Arrays");
    const size_t na = pb.max_actors;
    if ((clocks && n_clocks != n * na) || (prefix && n_prefix != n)) return throw_msg(env, "batchAtVersions: clocks holds maxActors entries per cut, prefix one");
    const bool diff = u32_prop(env, argv[2], "diff", 0u) != 0u, then_rest = diff || u32_prop(env, argv[2], "thenRest", 0u) != 0u;
    /* strings (optional): a stringsUpload handle — the text of the cut logs comes back with their result, as resultText returns it */
    ptx_dstrings* ds = nullptr;
    {
        napi_value sv;
        bool has = false;
        if (napi_has_named_property(env, argv[2], "strings", &has) == napi_ok && has && napi_get_named_property(env, argv[2], "strings", &sv) == napi_ok) ds = strings_of(env, sv);
    }
    ptx_text text;
    memset(&text, 0, sizeof(text));
    std::vector<uint32_t> out((5 + na) * n + 1, 0); /* status | nKept | firstRow | clocksOut */
    uint32_t none = 0; /* (a zero-length ArrayBuffer may come without storage) */
    ptx_dbatch *db = nullptr, *cut = nullptr;
    ptx_dresult* dr = nullptr;
    ptx_host_batch hb;
    ptx_result res;
    ptx_patches pat;
    memset(&hb, 0, sizeof(hb));
    memset(&pat, 0, sizeof(pat));
    bool have_res = false;
    ptx_status st = L.batch_upload(ctx, &pb, &db);
    if (st == PTX_OK)
        st = L.batch_at_versions(ctx, db, (uint32_t)n, n ? (const uint32_t*)src : &none, (const uint32_t*)clocks, (const uint32_t*)prefix, then_rest ? PTX_VERSIONS_THEN_REST : 0u, &cut,
                                 out.data(), out.data() + n, out.data() + 2 * n, out.data() + 3 * n);
    if (st == PTX_OK) st = L.batch_download(ctx, cut, &hb);
    if (st == PTX_OK) st = L.result_alloc(ctx, cut, &dr);
    if (st == PTX_OK) st = L.merge(ctx, cut, dr);
    if (st == PTX_OK) st = L.sync(ctx);
    if (st == PTX_OK) st = L.result_download(ctx, cut, dr, &res);
    have_res = st == PTX_OK;
    if (st == PTX_OK && ds) st = L.result_text_range(ctx, cut, dr, ds, 0, (uint32_t)n, &text);
    if (st == PTX_OK && diff) st = L.replay_patches_from(ctx, cut, dr, out.data() + 2 * n, &pat);
    std::string err = st != PTX_OK ? L.last_error(ctx) : "";
    if (dr) L.dresult_free(ctx, dr);
    if (cut) L.batch_free(ctx, cut);
    if (db) L.batch_free(ctx, db);
    if (st != PTX_OK) {
        if (have_res) L.result_free(&res);
        if (text.owner) L.text_free(&text);
        if (hb.owner) L.host_batch_free(&hb);
        char msg[1024];
        snprintf(msg, sizeof(msg), "ptx_batch_at_versions failed (status %d): %s", st, err.c_str());
        return throw_msg(env, msg);
    }
    napi_value o, v, batch = batch_to_js(env, hb.b);
    L.host_batch_free(&hb);
    napi_value result = result_to_js(env, res, diff ? &pat : nullptr);
    if (text.owner) {
        if (result) text_to_js(env, text, result);
        else L.text_free(&text);
    }
    if (!batch || !result || napi_create_object(env, &o) != napi_ok) return throw_msg(env, "batchAtVersions: cannot build the result object");
    napi_set_named_property(env, o, "batch", batch);
    napi_set_named_property(env, o, "result", result);
    const char* names[4] = {"status", "nKept", "firstRow", "clocksOut"};
    for (int k = 0; k < 4; ++k) {
        v = make_u32(env, out.data() + (size_t)k * n, k < 3 ? n : n * na);
        if (v) napi_set_named_property(env, o, names[k], v);
    }
    return o;
}

/* rootMap(ctx, batch): Micromerge.getRoot() for every replica log of the batch (ptx_root_map): upload, resolve.  Returns
 * {entryOff: BigUint64Array [n_logs + 1], logs: Uint32Array (status, n_entries, first_bad_row, 0 per log), entries: Uint32Array
 * (obj lo, obj hi, key, row, kind, value per entry)}. */
napi_value RootMap(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    if (argc < 2) return throw_msg(env, "rootMap(ctx, batch)");
    ptx_ctx* ctx = ctx_of(env, argv[0]);
    if (!ctx) return throw_msg(env, "rootMap: bad context");
    ptx_batch pb;
    if (!read_batch(env, argv[1], &pb)) return nullptr;
    ptx_dbatch* db = nullptr;
    ptx_root_maps rm;
    memset(&rm, 0, sizeof(rm));
    ptx_status st = L.batch_upload(ctx, &pb, &db);
    if (st == PTX_OK) st = L.root_map(ctx, db, &rm);
    if (db) L.batch_free(ctx, db);
    if (st != PTX_OK) {
        char msg[1024];
        snprintf(msg, sizeof(msg), "ptx_root_map failed (status %d): %s", st, L.last_error(ctx));
        return throw_msg(env, msg);
    }
    static_assert(sizeof(ptx_root_entry) == 24 && sizeof(ptx_root_log) == 16, "ptx_root_entry / ptx_root_log layout");
    napi_value out, v, ab, ta;
    NAPI_OK(napi_create_object(env, &out));
    void* data = nullptr;
    const size_t n_off = (size_t)rm.n_logs + 1;
    if (napi_create_arraybuffer(env, n_off * 8, &data, &ab) == napi_ok && napi_create_typedarray(env, napi_biguint64_array, n_off, ab, 0, &ta) == napi_ok) {
        memcpy(data, rm.entry_off, n_off * 8);
        napi_set_named_property(env, out, "entryOff", ta);
    }
    v = make_u32(env, rm.logs, (size_t)rm.n_logs * 4);
    if (v) napi_set_named_property(env, out, "logs", v);
    v = make_u32(env, rm.entries, (size_t)rm.entry_off[rm.n_logs] * 6);
    if (v) napi_set_named_property(env, out, "entries", v);
    L.root_maps_free(&rm);
    return out;
}

/* cursors(ctx, batch, {log: Uint32Array, kind: Uint8Array, arg: BigUint64Array}): Micromerge.getCursor / resolveCursor for many replicas
 * (ptx_resolve_cursors): upload, merge, resolve.  Returns {out: BigUint64Array, status: Uint32Array}, one entry per query. */
napi_value Cursors(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 2 ? ctx_of(env, argv[0]) : nullptr;
    if (!ctx) return throw_msg(env, "cursors(ctx, batch | resident handle, queries)");
    napi_valuetype vt;
    const bool resident = napi_typeof(env, argv[1], &vt) == napi_ok && vt == napi_external; /* the logs already in HBM: nothing is encoded or uploaded */
    ptx_batch pb;
    memset(&pb, 0, sizeof(pb));
    ptx_dbatch* rdb = resident ? dbatch_of(env, argv[1]) : nullptr;
    if (resident && !rdb) return throw_msg(env, "cursors: bad resident handle");
    if (!resident && !read_batch(env, argv[1], &pb)) return nullptr;
    const void *ql = nullptr, *qk = nullptr, *qa = nullptr;
    size_t n = 0, n2 = 0, n3 = 0;
    if (!column(env, argv[2], "log", 4, &ql, &n) || !column(env, argv[2], "kind", 1, &qk, &n2) || !column(env, argv[2], "arg", 8, &qa, &n3) || n != n2 || n != n3)
        return throw_msg(env, "cursors: queries = {log: Uint32Array, kind: Uint8Array, arg: BigUint64Array} of one length");
    std::vector<uint64_t> out(n ? n : 1);
    std::vector<uint32_t> status(n ? n : 1);
    ptx_dbatch* db = nullptr;
    ptx_dresult* dr = nullptr;
    ptx_status st = resident ? PTX_OK : L.batch_upload(ctx, &pb, &db);
    if (resident) db = rdb;
    if (st == PTX_OK) st = L.result_alloc(ctx, db, &dr);
    if (st == PTX_OK) st = L.merge(ctx, db, dr);
    if (st == PTX_OK) st = L.sync(ctx);
    if (st == PTX_OK) st = L.resolve_cursors(ctx, db, dr, (uint32_t)n, (const uint32_t*)ql, (const uint8_t*)qk, (const uint64_t*)qa, out.data(), status.data());
    std::string err = st != PTX_OK ? L.last_error(ctx) : "";
    if (dr) L.dresult_free(ctx, dr);
    if (db && !resident) L.batch_free(ctx, db);
    if (st != PTX_OK) return throw_msg(env, ("ptx_resolve_cursors failed: " + err).c_str());
    napi_value o, v;
    NAPI_OK(napi_create_object(env, &o));
    v = make_typed(env, napi_biguint64_array, 8, out.data(), n);
    if (v) napi_set_named_property(env, o, "out", v);
    v = make_u32(env, status.data(), n);
    if (v) napi_set_named_property(env, o, "status", v);
    return o;
}

/* commUniqueId(ctx) -> Uint8Array(128): rank 0 makes it, the host's own channel carries it to the other ranks */
napi_value CommUniqueId(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc ? ctx_of(env, argv[0]) : nullptr;
    if (!ctx) return throw_msg(env, "commUniqueId(ctx)");
    uint8_t id[PTX_COMM_ID_BYTES];
    if (L.comm_unique_id(ctx, id) != PTX_OK) return throw_msg(env, L.last_error(ctx));
    return make_typed(env, napi_uint8_array, 1, id, PTX_COMM_ID_BYTES);
}

/* commInit(ctx, id: Uint8Array(128), rank, nRanks) -> comm (external); collective over all ranks */
napi_value CommInit(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 4;
    napi_value argv[4];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 3 ? ctx_of(env, argv[0]) : nullptr;
    if (!ctx) return throw_msg(env, "commInit(ctx, id, rank, nRanks)");
    napi_typedarray_type type;
    size_t length = 0, offset = 0;
    void* data = nullptr;
    napi_value ab;
    if (napi_get_typedarray_info(env, argv[1], &type, &length, &data, &ab, &offset) != napi_ok || type != napi_uint8_array || length != PTX_COMM_ID_BYTES)
        return throw_msg(env, "commInit: id must be the Uint8Array(128) commUniqueId() made on rank 0");
    uint32_t rank = 0, n = 1;
    napi_get_value_uint32(env, argv[2], &rank);
    napi_get_value_uint32(env, argv[3], &n);
    ptx_comm* comm = nullptr;
    if (L.comm_init(ctx, (const uint8_t*)data, rank, n, &comm) != PTX_OK) return throw_msg(env, L.last_error(ctx));
    napi_value ext;
    NAPI_OK(napi_create_external(env, comm, nullptr, nullptr, &ext));
    return ext;
}

napi_value CommDestroy(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 1 ? ctx_of(env, argv[0]) : nullptr;
    void* p = nullptr;
    if (ctx && L.handle && napi_get_value_external(env, argv[1], &p) == napi_ok && p) L.comm_destroy(ctx, (ptx_comm*)p);
    return nullptr;
}

/* mergeAndGather(ctx, comm, batch, counts: Uint32Array(nRanks), replicas): this rank's replica logs are merged, the per-replica
 * digests of ALL ranks gathered on the device (ptx_allgather_digests) and the converged documents of the whole job counted there.
 * Returns {logs: Uint32Array (this rank's ptx_log_result rows), gathered: BigUint64Array (2 per replica log, rank-major), converged}. */
napi_value MergeAndGather(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 5;
    napi_value argv[5];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 4 ? ctx_of(env, argv[0]) : nullptr;
    void* cp = nullptr;
    if (!ctx || napi_get_value_external(env, argv[1], &cp) != napi_ok || !cp) return throw_msg(env, "mergeAndGather(ctx, comm, batch, counts, replicas)");
    ptx_batch pb;
    if (!read_batch(env, argv[2], &pb)) return nullptr;
    napi_typedarray_type type;
    size_t n_ranks = 0, offset = 0;
    void* counts = nullptr;
    napi_value ab;
    if (napi_get_typedarray_info(env, argv[3], &type, &n_ranks, &counts, &ab, &offset) != napi_ok || type != napi_uint32_array || n_ranks == 0)
        return throw_msg(env, "mergeAndGather: counts must be a Uint32Array with one entry per rank");
    if (n_ranks != L.comm_n_ranks((const ptx_comm*)cp)) return throw_msg(env, "mergeAndGather: counts.length differs from the communicator's rank count");
    uint32_t replicas = 1;
    napi_get_value_uint32(env, argv[4], &replicas);
    uint64_t total = 0;
    for (size_t k = 0; k < n_ranks; ++k) total += ((const uint32_t*)counts)[k];
    ptx_dbatch* db = nullptr;
    ptx_dresult* dr = nullptr;
    void *d_gather = nullptr, *d_count = nullptr;
    std::vector<ptx_log_result> logs(pb.n_logs ? pb.n_logs : 1);
    std::vector<uint64_t> gathered(total * 2 + 1);
    uint64_t converged = 0;
    ptx_status st = L.batch_upload(ctx, &pb, &db);
    if (st == PTX_OK) st = L.result_alloc(ctx, db, &dr);
    if (st == PTX_OK) st = L.device_alloc(ctx, total * 16 + 16, &d_gather);
    if (st == PTX_OK) st = L.device_alloc(ctx, 8, &d_count);
    if (st == PTX_OK) st = L.merge(ctx, db, dr);
    if (st == PTX_OK) st = L.allgather_digests(ctx, (ptx_comm*)cp, dr, (const uint32_t*)counts, (uint64_t*)d_gather);
    if (st == PTX_OK) st = L.count_converged_digests(ctx, (const uint64_t*)d_gather, total, replicas, (uint64_t*)d_count);
    if (st == PTX_OK) st = L.result_download_logs(ctx, dr, logs.data(), pb.n_logs);
    if (st == PTX_OK) st = L.device_read(ctx, d_gather, gathered.data(), total * 16);
    if (st == PTX_OK) st = L.device_read(ctx, d_count, &converged, 8);
    std::string err = st != PTX_OK ? L.last_error(ctx) : "";
    if (d_gather) L.device_free(ctx, d_gather);
    if (d_count) L.device_free(ctx, d_count);
    if (dr) L.dresult_free(ctx, dr);
    if (db) L.batch_free(ctx, db);
    if (st != PTX_OK) return throw_msg(env, ("mergeAndGather failed: " + err).c_str());
    napi_value out, v;
    NAPI_OK(napi_create_object(env, &out));
    v = make_u32(env, logs.data(), (size_t)pb.n_logs * 12);
    if (v) napi_set_named_property(env, out, "logs", v);
    v = make_typed(env, napi_biguint64_array, 8, gathered.data(), (size_t)total * 2);
    if (v) napi_set_named_property(env, out, "gathered", v);
    napi_create_double(env, (double)converged, &v);
    napi_set_named_property(env, out, "converged", v);
    return out;
}

/* accumulatePatches(ctx, batch, streams: {patchOff: BigUint64Array(nLogs + 1), patchLogs: Uint32Array(2 per log), patches: Uint32Array(4 per record)}) -> the
 * result object of applyMaterialize (no elemRank): the documents the streams describe (ptx_accumulate_patches) */
napi_value AccumulatePatches(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 2 ? ctx_of(env, argv[0]) : nullptr;
    if (!ctx) return throw_msg(env, "accumulatePatches(ctx, batch, streams)");
    ptx_batch pb;
    if (!read_batch(env, argv[1], &pb)) return nullptr;
    const void *off = nullptr, *logs = nullptr, *recs = nullptr;
    size_t n_off = 0, n_logs = 0, n_recs = 0;
    if (!column(env, argv[2], "patchOff", 8, &off, &n_off) || !column(env, argv[2], "patchLogs", 4, &logs, &n_logs) || !column(env, argv[2], "patches", 4, &recs, &n_recs) ||
        n_off != (size_t)pb.n_logs + 1 || n_logs != (size_t)pb.n_logs * 2 || (uint64_t)n_recs < ((const uint64_t*)off)[pb.n_logs] * 4)
        return throw_msg(env, "accumulatePatches: streams need patchOff (BigUint64Array, nLogs + 1), patchLogs (Uint32Array, 2 per log) and patches (Uint32Array, 4 per record)");
    ptx_patches pat;
    memset(&pat, 0, sizeof(pat));
    pat.n_logs = pb.n_logs;
    pat.patch_off = (const uint64_t*)off;
    pat.logs = (const ptx_patch_log*)logs;
    pat.patches = (const ptx_patch*)recs;
    ptx_dbatch* db = nullptr;
    ptx_result res;
    ptx_status st = L.batch_upload(ctx, &pb, &db);
    if (st == PTX_OK) st = L.accumulate_patches(ctx, db, &pat, &res);
    std::string err = st != PTX_OK ? L.last_error(ctx) : "";
    if (db) L.batch_free(ctx, db);
    if (st != PTX_OK) return throw_msg(env, ("accumulatePatches failed: " + err).c_str());
    return result_to_js(env, res, nullptr);
}

/* checkPatches(ctx, batch) -> {rows: Uint32Array (8 per log: status, agrees, nPatches, firstBadRecord, digest as 4 x u32), disagree}: merge, replay and
 * accumulate on the device, the streams compared with the merge there (ptx_check_patches) */
napi_value CheckPatches(napi_env env, napi_callback_info info) {
    if (!L.handle) return throw_msg(env, "call open(libPath) first");
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc > 1 ? ctx_of(env, argv[0]) : nullptr;
    if (!ctx) return throw_msg(env, "checkPatches(ctx, batch)");
    ptx_batch pb;
    if (!read_batch(env, argv[1], &pb)) return nullptr;
    static_assert(sizeof(ptx_patch_check_log) == 32, "ptx_patch_check_log layout");
    std::vector<ptx_patch_check_log> rows(pb.n_logs ? pb.n_logs : 1);
    uint64_t disagree = 0;
    ptx_dbatch* db = nullptr;
    ptx_dresult* dr = nullptr;
    ptx_status st = L.batch_upload(ctx, &pb, &db);
    if (st == PTX_OK) st = L.result_alloc(ctx, db, &dr);
    if (st == PTX_OK) st = L.merge(ctx, db, dr);
    if (st == PTX_OK) st = L.sync(ctx);
    if (st == PTX_OK) st = L.check_patches(ctx, db, dr, rows.data(), &disagree);
    std::string err = st != PTX_OK ? L.last_error(ctx) : "";
    if (dr) L.dresult_free(ctx, dr);
    if (db) L.batch_free(ctx, db);
    if (st != PTX_OK) return throw_msg(env, ("checkPatches failed: " + err).c_str());
    napi_value out, v;
    NAPI_OK(napi_create_object(env, &out));
    v = make_u32(env, rows.data(), (size_t)pb.n_logs * 8);
    if (v) napi_set_named_property(env, out, "rows", v);
    napi_create_double(env, (double)disagree, &v);
    napi_set_named_property(env, out, "disagree", v);
    return out;
}

napi_value MaxOpsPerLog(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ptx_ctx* ctx = argc ? ctx_of(env, argv[0]) : nullptr;
    napi_value v;
    NAPI_OK(napi_create_uint32(env, L.handle ? L.max_ops_per_log(ctx) : 0, &v));
    return v;
}

napi_value KernelName(napi_env env, napi_callback_info) {
    napi_value v;
    NAPI_OK(napi_create_string_utf8(env, L.handle ? L.kernel_name() : "", NAPI_AUTO_LENGTH, &v));
    return v;
}

napi_value Init(napi_env env, napi_value exports) {
    struct { const char* name; napi_callback fn; } fns[] = {
        {"open", Open}, {"create", Create}, {"destroy", Destroy}, {"applyMaterialize", ApplyMaterialize}, {"residentUpload", ResidentUpload}, {"residentAppend", ResidentAppend}, {"residentApply", ResidentApply}, {"residentFree", ResidentFree}, {"generate", Generate}, {"change", Change}, {"cursors", Cursors}, {"rootMap", RootMap}, {"commUniqueId", CommUniqueId}, {"commInit", CommInit}, {"commDestroy", CommDestroy}, {"mergeAndGather", MergeAndGather},
        {"maxOpsPerLog", MaxOpsPerLog}, {"kernelName", KernelName},
    };
    for (auto& f : fns) {
        napi_value fn;
        if (napi_create_function(env, f.name, NAPI_AUTO_LENGTH, f.fn, nullptr, &fn) != napi_ok) return nullptr;
        if (napi_set_named_property(env, exports, f.name, fn) != napi_ok) return nullptr;
    }
    /* the enumerable exports above are the list the host's load check pins (tests/test_node_host.py); entry points added since are defined beside them as plain
     * (non-enumerable) properties: index.js calls them by name */
    const napi_property_descriptor later[] = {{"syncReplicas", nullptr, SyncReplicas, nullptr, nullptr, nullptr, napi_default, nullptr},
                                              {"accumulatePatches", nullptr, AccumulatePatches, nullptr, nullptr, nullptr, napi_default, nullptr},
                                              {"checkPatches", nullptr, CheckPatches, nullptr, nullptr, nullptr, napi_default, nullptr},
                                              {"batchAtVersions", nullptr, BatchAtVersions, nullptr, nullptr, nullptr, napi_default, nullptr},
                                              {"stringsUpload", nullptr, StringsUpload, nullptr, nullptr, nullptr, napi_default, nullptr},
                                              {"stringsFree", nullptr, StringsFree, nullptr, nullptr, nullptr, napi_default, nullptr},
                                              {"resultText", nullptr, ResultText, nullptr, nullptr, nullptr, napi_default, nullptr},
                                              {"findText", nullptr, FindText, nullptr, nullptr, nullptr, napi_default, nullptr},
                                              {"textSlices", nullptr, TextSlices, nullptr, nullptr, nullptr, napi_default, nullptr},
                                              {"viewCreate", nullptr, ViewCreate, nullptr, nullptr, nullptr, napi_default, nullptr},
                                              {"viewFree", nullptr, ViewFree, nullptr, nullptr, nullptr, napi_default, nullptr},
                                              {"viewFindText", nullptr, ViewFindText, nullptr, nullptr, nullptr, napi_default, nullptr},
                                              {"viewTextSlices", nullptr, ViewTextSlices, nullptr, nullptr, nullptr, napi_default, nullptr},
                                              {"viewFindSnippets", nullptr, ViewFindSnippets, nullptr, nullptr, nullptr, napi_default, nullptr},
                                              {"viewReplacePlan", nullptr, ViewReplacePlan, nullptr, nullptr, nullptr, napi_default, nullptr},
                                              {"viewMarkRuns", nullptr, ViewMarkRuns, nullptr, nullptr, nullptr, napi_default, nullptr},
                                              {"viewMarkSnippets", nullptr, ViewMarkSnippets, nullptr, nullptr, nullptr, napi_default, nullptr},
                                              {"viewFindInMarks", nullptr, ViewFindInMarks, nullptr, nullptr, nullptr, napi_default, nullptr}};
    if (napi_define_properties(env, exports, sizeof(later) / sizeof(later[0]), later) != napi_ok) return nullptr;
    return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
