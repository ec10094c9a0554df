#include "ThreadGrid.h"

#include <cstdio>
#include <cstring>

namespace ohm_tsd_slam
{

ThreadGrid::ThreadGrid(obvious::TsdGrid* grid, const std::shared_ptr<rclcpp::Node>& node, const double xOffset, const double yOffset):
    ThreadSLAM(*grid),
    _node(node),
    _occGrid(std::make_shared<nav_msgs::msg::OccupancyGrid>()),
    _width(grid->getCellsX()),
    _height(grid->getCellsY()),
    _cellSize(grid->getCellSize()),
    _hOcc(nullptr),
    _hRgb(nullptr),
    _frames(0)
{
  // (ThreadGrid.cpp:16-40)
  _occGrid->info.resolution           = static_cast<double>(_grid.getCellSize());
  _occGrid->info.width                = _grid.getCellsX();
  _occGrid->info.height               = _grid.getCellsY();
  _occGrid->info.origin.orientation.w = 1.0;
  _occGrid->info.origin.orientation.x = 0.0;
  _occGrid->info.origin.orientation.y = 0.0;
  _occGrid->info.origin.orientation.z = 0.0;
  _occGrid->info.origin.position.x    = -(static_cast<double>(_grid.getCellsX()) * static_cast<double>(_grid.getCellSize()) * 0.5 + xOffset);
  _occGrid->info.origin.position.y    = -(static_cast<double>(_grid.getCellsY()) * static_cast<double>(_grid.getCellSize()) * 0.5 + yOffset);
  _occGrid->info.origin.position.z    = 0.0;
  _occGrid->data.resize((size_t)_width * _height);

  // pub_tsd_color_map / object_inflation_factor / use_object_inflation are declared with the node's parameters
  // (facade_capi.cpp: declare_node_parameters), so they are only read here (ThreadGrid.cpp:42-53).  The reference never reads
  // pub_tsd_color_map: the image is published with every map.
  _occGrid->header.frame_id = node->get_parameter("tf_map_frame").as_string();
  _objectInflation = node->get_parameter("use_object_inflation").as_bool();
  _objInflateFactor = static_cast<unsigned int>(node->get_parameter("object_inflation_factor").as_int());

  const std::string node_name = _node->get_name();
  _gridPub = node->create_publisher<nav_msgs::msg::OccupancyGrid>(node_name + "/map", rclcpp::QoS(1).reliable().transient_local());
  _pubColorImage = node->create_publisher<sensor_msgs::msg::Image>(node_name + "/map/image", rclcpp::QoS(1).best_effort());
  _getMapServ = node->create_service<nav_msgs::srv::GetMap>(
    node_name + "/get_map",
    std::bind(&ThreadGrid::getMapServCallBack, this, std::placeholders::_1, std::placeholders::_2));

  // (ThreadGrid.cpp:64-68)
  _image.header.frame_id = "map";
  _image.step = _grid.getCellsY() * 3;
  _image.data.resize((size_t)_width * _height * 3);
  startThread();
}

ThreadGrid::~ThreadGrid()
{
  // (a publication in progress finishes first: publish() waits for its frame before it returns)
  terminateThread();
  joinThread();
  tsd_host_free(_hOcc);
  tsd_host_free(_hRgb);
}

uint64_t ThreadGrid::frames(void)
{
  std::lock_guard<std::mutex> lk(_msgMutex);
  return _frames;
}

void ThreadGrid::eventLoop(void)
{
  while(_stayActive)
  {
    waitForWork();
    if(!_stayActive)
      break;
    publish();
  }
}

int ThreadGrid::publish(void)
{
  std::lock_guard<std::mutex> lk(_publishMutex);
  const size_t cells = (size_t)_width * _height;
  if(!_hOcc)                   // (allocated at the first publication: a node that never publishes pins nothing)
  {
    _hOcc = static_cast<int8_t*>(tsd_host_alloc(cells));
    _hRgb = static_cast<uint8_t*>(tsd_host_alloc(3 * cells));
  }
  if(!_hOcc || !_hRgb)
    return TSD_E_ARG;
  tsd_ctx* ctx = _grid.context();
  tsd_map_params prm;
  prm.inflate = _objectInflation ? 1 : 0;
  prm.inflate_factor = static_cast<int32_t>(_objInflateFactor);
  int rc;
  {
    // the grid's mutex only while the frame is enqueued: the localisers go on while it is computed and copied
    std::lock_guard<std::mutex> g(_grid.mutex());
    rc = tsd_map_frame_begin(ctx, &prm, _hOcc, _hRgb);
  }
  if(rc != TSD_OK)
    return rc;
  int mapSize2 = 0;          // calcCoords' mapSize / 2
  rc = tsd_map_frame_wait(ctx, &mapSize2);
  if(rc != TSD_OK)
    return rc;
  if(mapSize2 == 0)
  {
#if OHM_TSD_SLAM_HAVE_ROS
    RCLCPP_WARN(_node->get_logger(), "OccupancyGridThread: Warning! Raycasting returned with no coordinates, map contains no data yet!\n");
#else
    std::fprintf(stderr, "OccupancyGridThread: Warning! Raycasting returned with no coordinates, map contains no data yet!\n");
#endif
  }
  nav_msgs::msg::OccupancyGrid msg;
  {
    std::lock_guard<std::mutex> m(_msgMutex);
    _occGrid->header.stamp       = _node->get_clock()->now();
    _occGrid->info.map_load_time = _node->get_clock()->now();
    std::memcpy(_occGrid->data.data(), _hOcc, cells);
    msg = *_occGrid;
    _frames++;
  }
  _gridPub->publish(msg);
  // (ThreadGrid.cpp:120-131)
  _image.header.stamp = msg.header.stamp;
  _image.height = msg.info.height;
  _image.width = msg.info.width;
  _image.encoding = sensor_msgs::image_encodings::RGB8;
  std::memcpy(_image.data.data(), _hRgb, 3 * cells);
  _pubColorImage->publish(_image);
  return TSD_OK;
}

bool ThreadGrid::getMapServCallBack(const std::shared_ptr<nav_msgs::srv::GetMap::Request>,
                                    std::shared_ptr<nav_msgs::srv::GetMap::Response> res)
{
  std::lock_guard<std::mutex> m(_msgMutex);
  res->map = *_occGrid;
  res->map.header.stamp = _node->get_clock()->now();
  _occGrid->info.map_load_time = _node->get_clock()->now();
  return true;
}

} /* namespace ohm_tsd_slam */
