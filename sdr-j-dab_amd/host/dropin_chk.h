// dropin_chk.h -- private to the drop-in library's sources: a failing C ABI call throws dabgpu::error
#pragma once
#include <string>

#include "dabgpu_dropin.h"

namespace dabgpu {

inline void chk(int rc, const char *what) {
    if (rc != DABGPU_OK) throw error(rc, std::string(what) + ": " + dabgpu_last_error());
}

}  // namespace dabgpu
