// owned byte buffer handed across the C ABI by the builders (ds2i_build.h: ds2i_blob_*)
#pragma once
#include <cstdint>
#include <memory>
#include <vector>
struct ds2i_blob { std::vector<uint8_t> data; };
// a vector's bytes as a fresh blob
template <class T>
ds2i_blob* ds2i_blob_of(std::vector<T> const& v) {
    std::unique_ptr<ds2i_blob> b(new ds2i_blob);
    const uint8_t* p = (const uint8_t*)v.data();
    b->data.assign(p, p + sizeof(T) * v.size());
    return b.release();
}
