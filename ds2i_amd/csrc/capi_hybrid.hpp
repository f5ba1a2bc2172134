// the ds2i_hybrid handle, shared by its host entry points (capi_build.cpp) and its GPU ones (capi_encode.cpp)
#pragma once
#include <memory>

#include "host_hybrid.hpp"

struct ds2i_hybrid {
    std::unique_ptr<ds2i_host::hybrid_index_builder> b;
};
