#pragma once
#include "kai_handle.hpp"
namespace {
// RCCL, resolved at run time (the library loads without it; only kai_shard_attach_rccl needs it).  Prototypes as in rccl/rccl.h: ncclUniqueId is 128 opaque bytes passed BY VALUE,
// ncclUint8 = 1, ncclSuccess = 0.
struct RcclId { char internal[128]; };
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(RcclId*) = nullptr;
    int (*CommInitRank)(void**, int, RcclId, int) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
RcclApi* rccl_api() {
    static RcclApi a; static bool tried = false;
    if (!tried) {
        tried = true;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { a.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL); if (a.lib) break; }
        if (a.lib) {
            a.GetUniqueId = reinterpret_cast<int (*)(RcclId*)>(dlsym(a.lib, "ncclGetUniqueId"));
            a.CommInitRank = reinterpret_cast<int (*)(void**, int, RcclId, int)>(dlsym(a.lib, "ncclCommInitRank"));
            a.AllGather = reinterpret_cast<int (*)(const void*, void*, size_t, int, void*, hipStream_t)>(dlsym(a.lib, "ncclAllGather"));
            a.CommDestroy = reinterpret_cast<int (*)(void*)>(dlsym(a.lib, "ncclCommDestroy"));
            a.GetErrorString = reinterpret_cast<const char* (*)(int)>(dlsym(a.lib, "ncclGetErrorString"));
        }
    }
    return (a.lib && a.GetUniqueId && a.CommInitRank && a.AllGather && a.CommDestroy) ? &a : nullptr;
}
int rccl_fail(kai_core* core, const char* what, int rc) {
    RcclApi* a = rccl_api();
    core->err = std::string(what) + ": " + ((a && a->GetErrorString) ? a->GetErrorString(rc) : "RCCL error");
    return KAI_ERR_COMM;
}
}  // namespace
