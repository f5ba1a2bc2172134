// the ds2i_hybrid handle, shared by its host entry points (capi_build.cpp) and its GPU ones (capi_encode.cpp), and the decode-time
// model in its two forms: the published ds2i_hybrid_model and the optimiser's hybrid_model, six floats each
#pragma once
#include <memory>

#include "../../include/ds2i_build.h"
#include "host_hybrid.hpp"

struct ds2i_hybrid {
    std::unique_ptr<ds2i_host::hybrid_index_builder> b;
};

inline ds2i_host::hybrid_model to_model(const ds2i_hybrid_model* model) { // (null = the default model)
    ds2i_host::hybrid_model m;
    if (model) {
        m.pfor_base = model->pfor_base; m.pfor_exc = model->pfor_exc; m.pfor_exc_many = model->pfor_exc_many;
        m.varint = model->varint; m.interp_base = model->interp_base; m.interp_node = model->interp_node;
    }
    return m;
}
inline ds2i_hybrid_model from_model(ds2i_host::hybrid_model const& m) {
    return ds2i_hybrid_model{m.pfor_base, m.pfor_exc, m.pfor_exc_many, m.varint, m.interp_base, m.interp_node};
}
