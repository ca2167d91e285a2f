// Stand-in for the receiver's GUI class: motHandler only connects its signal to it.
#ifndef MOT_STUB_GUI
#define MOT_STUB_GUI
class RadioInterface {};
#endif
