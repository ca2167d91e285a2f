/* Stand-in for <portaudio.h>: the declarations audiosink.cpp uses; sink_golden_driver.cpp defines
 * them as one silent output device whose stream never calls back on its own.  Used only by
 * tests/golden/make_sink_golden.py. */
#ifndef SINK_STUB_PORTAUDIO
#define SINK_STUB_PORTAUDIO
typedef int PaError;
typedef int PaDeviceIndex;
typedef int PaHostApiIndex;
typedef double PaTime;
typedef unsigned long PaSampleFormat;
typedef unsigned long PaStreamCallbackFlags;
typedef void PaStream;
enum { paNoError = 0, paFormatIsSupported = 0 };
enum { paContinue = 0, paComplete = 1, paAbort = 2 };
#define paFloat32 ((PaSampleFormat)0x00000001)
typedef struct { const char *name; } PaHostApiInfo;
typedef struct {
    const char *name;
    int maxInputChannels, maxOutputChannels;
    PaTime defaultLowOutputLatency, defaultHighOutputLatency;
} PaDeviceInfo;
typedef struct {
    PaDeviceIndex device;
    int channelCount;
    PaSampleFormat sampleFormat;
    PaTime suggestedLatency;
    void *hostApiSpecificStreamInfo;
} PaStreamParameters;
typedef struct { PaTime inputBufferAdcTime, currentTime, outputBufferDacTime; } PaStreamCallbackTimeInfo;
typedef int PaStreamCallback(const void *, void *, unsigned long, const PaStreamCallbackTimeInfo *, PaStreamCallbackFlags, void *);
PaError Pa_Initialize(void);
PaError Pa_Terminate(void);
PaHostApiIndex Pa_GetHostApiCount(void);
const PaHostApiInfo *Pa_GetHostApiInfo(PaHostApiIndex);
PaDeviceIndex Pa_GetDeviceCount(void);
PaDeviceIndex Pa_GetDefaultOutputDevice(void);
const PaDeviceInfo *Pa_GetDeviceInfo(PaDeviceIndex);
PaError Pa_IsFormatSupported(const PaStreamParameters *, const PaStreamParameters *, double);
PaError Pa_OpenStream(PaStream **, const PaStreamParameters *, const PaStreamParameters *, double, unsigned long, unsigned long,
                      PaStreamCallback *, void *);
PaError Pa_CloseStream(PaStream *);
PaError Pa_StartStream(PaStream *);
PaError Pa_StopStream(PaStream *);
PaError Pa_AbortStream(PaStream *);
PaError Pa_IsStreamStopped(PaStream *);
void Pa_Sleep(long);
#endif
