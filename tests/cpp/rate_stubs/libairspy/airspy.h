// TEST INFRASTRUCTURE: the types of libairspy's interface that airspy-handler.{h,cpp} name.  The
// functions themselves are the driver's (rate_golden_driver.cpp hands them out through dlsym).
#pragma once
#include <stdint.h>
#include <stdlib.h>
struct airspy_device;
enum airspy_error { AIRSPY_SUCCESS = 0, AIRSPY_ERROR_OTHER = -9999 };
enum airspy_board_id { AIRSPY_BOARD_ID_PROTO_AIRSPY = 0 };
enum airspy_sample_type { AIRSPY_SAMPLE_FLOAT32_IQ = 0, AIRSPY_SAMPLE_INT16_IQ = 2 };
typedef struct airspy_transfer {
    struct airspy_device *device;
    void *ctx;
    void *samples;
    int sample_count;
    uint64_t dropped_samples;
    enum airspy_sample_type sample_type;
} airspy_transfer_t, airspy_transfer;
typedef struct {
    uint32_t part_id[2];
    uint32_t serial_no[4];
} airspy_read_partid_serialno_t;
typedef int (*airspy_sample_block_cb_fn)(airspy_transfer *transfer);
// the handler takes abs of a difference of uint32_t rates, which no overload of abs accepts
inline int abs(uint32_t x) { return ::abs((int)x); }
