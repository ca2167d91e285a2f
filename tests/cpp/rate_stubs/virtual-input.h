// TEST INFRASTRUCTURE: the base class of the reference's input handlers, with nothing behind it
#pragma once
#include <stdint.h>
#include "dab-constants.h"
#include <QObject>
#define AIRSPY 0111
class virtualInput : public QObject {
public:
    virtualInput() : lastFrequency(0), vfoOffset(0) {}
    virtual ~virtualInput() {}
    virtual void setVFOFrequency(int32_t) {}
    virtual int32_t getVFOFrequency() { return 0; }
    virtual uint8_t myIdentity() { return 0; }
    virtual bool legalFrequency(int32_t) { return true; }
    virtual int32_t defaultFrequency() { return 0; }
    virtual bool restartReader() { return true; }
    virtual void stopReader() {}
    virtual int32_t getSamples(DSPCOMPLEX *, int32_t) { return 0; }
    virtual int32_t Samples() { return 0; }
    virtual void resetBuffer() {}
    virtual int16_t bitDepth() { return 10; }
protected:
    int32_t lastFrequency;
    int32_t vfoOffset;
};
