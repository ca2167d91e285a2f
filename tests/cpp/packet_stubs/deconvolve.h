// Stand-in for the deconvolvers: the handler is given decoded bits, these are only constructed.
#ifndef PACKET_STUB_DECONVOLVE
#define PACKET_STUB_DECONVOLVE
#include <stdint.h>
class uep_deconvolve {
public:
    uep_deconvolve(int16_t, int16_t) {}
    bool deconvolve(int16_t *, int32_t, uint8_t *) { return true; }
};
class eep_deconvolve {
public:
    eep_deconvolve(int16_t, int16_t) {}
    bool deconvolve(int16_t *, int32_t, uint8_t *) { return true; }
};
#endif
