// twin_env.h -- what the host twins (inflate_twin.cpp, gzip_twin.cpp; g++) share: the sequential form of the decoder's
// environment (inflate_core.h) without its output side, and the CRC-32 table.  TEST INFRASTRUCTURE, not part of the product library.
#pragma once
#include "inflate_core.h"

// one lane, no barrier, the tables in the object itself
struct TwinTabs {
    uint32_t lane = 0, nl = 1;
    InfCode tabs[3];
    InfCode *lt = &tabs[0], *dt = &tabs[1], *ct = &tabs[2];
    uint8_t lens[320];
    void sync() {}
};

struct CrcTab { uint32_t t[256]; CrcTab() { inf_crc_table(t, 0, 1); } };
