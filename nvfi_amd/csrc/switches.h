// switches.h - every environment variable the library reads, one row each: name, kind, default.
// INT rows are parsed with atoi (a flag is an INT whose users ask `!= 0`); a WORD row takes one of the words below.  What a switch selects and
// the measurement behind its default stand where it is used; INTEGRATION.md section 4 is the user's table, and tests/test_abi_and_host.py
// holds the two together.
#pragma once

#define NVFI_SWITCHES(X)              \
    X(NVFI_SCATTER, WORD, mfma)       \
    X(NVFI_SCATTER_TILES, INT, 1)     \
    X(NVFI_DETERMINISTIC, INT, 0)     \
    X(NVFI_SIDE_STREAM, INT, 0)       \
    X(NVFI_FUSED_LAUNCH, INT, 1)      \
    X(NVFI_INTEGRATE_X6, INT, 1)      \
    X(NVFI_RK2_X6, INT, 1)            \
    X(NVFI_RK2_FUSE, INT, 1)          \
    X(NVFI_RK2_X4, INT, 1)            \
    X(NVFI_FUSE_X6, INT, 1)           \
    X(NVFI_PDE_FUSE, INT, 1)          \
    X(NVFI_PDE_PREFILTER, WORD, x6)   \
    X(NVFI_PDE_JET_X6, INT, 1)        \
    X(NVFI_X6W, INT, 1)               \
    X(NVFI_X6W_UNI, INT, 1)           \
    X(NVFI_X6W_MIN_TILES, INT, 4096)

enum Switch {
#define X(name, kind, def) name,
    NVFI_SWITCHES(X)
#undef X
    NVFI_SWITCH_COUNT
};
// values of the WORD rows.  NVFI_SCATTER: "lds", anything else is mfma.  NVFI_PDE_PREFILTER: "split32" reads as fp32, any other word as
// PRE_UNKNOWN, which pde.hip refuses
enum { SCATTER_LDS = 0, SCATTER_MFMA = 1 };
enum { PRE_UNKNOWN = -1, PRE_FP16BAND = 1, PRE_FP32 = 2, PRE_SPLIT16BAND = 3, PRE_X6 = 4 };

int sw(Switch s);   // the switch's value: the environment is read once per process, under a lock (abi.hip)
